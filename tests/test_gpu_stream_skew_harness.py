"""The skewed-stream harness (tests/stream_skew.py) on planted defects: a toy call with the library's pattern -- a producer copy on
the caller's stream S, a consumer on a second stream T, the result read on S -- with its fork, or its join, left out.  torch ops
only, and every read is of allocated memory: a planted defect reads poison, nothing can fault.

Whether the UNSKEWED run of a planted defect happens to pass is not asserted: with idle streams it usually does, which is why the
stream contract needs the skews."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import os  # noqa: E402
import sys  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stream_skew as K  # noqa: E402

N = 1 << 16
SKEWS = ((), ("main",), ("side",), ("main", "side"))


class Toy:
    """src --copy on S--> buf --(fork) x 2 + 1 on T--> mid --(join) copy on S--> out"""

    def __init__(self, fork=True, join=True):
        self.fork, self.join = fork, join
        self.S = torch.cuda.Stream()
        self.T, beside = K.caller_stream_beside([self.S])      # not on S's hardware queue, or a held T holds S back as well
        assert beside, "no second stream that runs beside the first: the planted defects cannot show"
        self.pristine = torch.arange(N, dtype=torch.float32, device="cuda") / 7
        self.src, self.buf, self.mid, self.out = (torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(4))
        self.ev_fork, self.ev_join = torch.cuda.Event(), torch.cuda.Event()
        torch.cuda.synchronize()

    def call(self):
        S, T = self.S, self.T
        self.buf.copy_(self.src)                      # producer, on S (the current stream)
        if self.fork:
            self.ev_fork.record(S)
            T.wait_event(self.ev_fork)
        with torch.cuda.stream(T):                    # consumer, on T
            torch.mul(self.buf, 2, out=self.mid)
            self.mid.add_(1)
        if self.join:
            self.ev_join.record(T)
            S.wait_event(self.ev_join)
        self.out.copy_(self.mid)                      # the result, read on S

    def run(self, skew, fill, hold_ms):
        return K.digest(K.run_skewed(self.call, {"src": (self.src, self.pristine)}, {"out": self.out}, [self.buf, self.mid], skew,
                                     self.S, fill=fill, hold_ms=hold_ms, sides={"side": self.T}))

    def hold_ms(self):
        return K.hold_ms_for(K.wall_ms(self.call, {"src": (self.src, self.pristine)}, self.S))


def expected():
    want = torch.arange(N, dtype=torch.float32, device="cuda") / 7 * 2 + 1
    return K.digest({"out": K.as_bytes(want)})


def test_hold_is_finite_and_about_as_long_as_asked():
    s = torch.cuda.Stream()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    K.cycles_per_ms()
    a.record(s)
    ev = K.hold(s, 50.0)
    b.record(s)
    assert not ev.query(), "a 50 ms hold was over when hold() returned"
    ev.synchronize()                                 # ends by itself
    b.synchronize()
    ms = a.elapsed_time(b)
    print(f"hold(50 ms) took {ms:.1f} ms at {K.cycles_per_ms():.0f} cycles per ms")
    assert 40.0 <= ms <= 100.0, ms                   # the calibration holds to 20 % down; up, a busy machine may double it


def test_correct_toy_call_is_clean_under_every_skew():
    toy = Toy()
    ms = toy.hold_ms()
    want = expected()
    for fill in K.FILLS:
        for skew in SKEWS:
            assert toy.run(skew, fill, ms) == want, (skew, hex(fill))


@pytest.mark.parametrize("fill", K.FILLS, ids=[f"fill{f:02X}" for f in K.FILLS])
def test_missing_fork_is_caught_by_the_main_skew(fill):
    toy = Toy(fork=False)
    assert toy.run(("main",), fill, toy.hold_ms()) != expected(), "the consumer ran before the producer and nobody noticed"


@pytest.mark.parametrize("fill", K.FILLS, ids=[f"fill{f:02X}" for f in K.FILLS])
def test_missing_join_is_caught_by_the_side_skew(fill):
    toy = Toy(join=False)
    assert toy.run(("side",), fill, toy.hold_ms()) != expected(), "the result was read before the consumer ran and nobody noticed"


def test_a_hold_that_is_too_short_fails_the_run():
    toy = Toy()
    with pytest.raises(AssertionError, match="the skew was not real"):
        K.run_skewed([toy.call, torch.cuda.synchronize], {"src": (toy.src, toy.pristine)}, {"out": toy.out}, [toy.buf, toy.mid],
                     ("side",), toy.S, hold_ms=1.0, sides={"side": toy.T})
