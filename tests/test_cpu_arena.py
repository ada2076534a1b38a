"""Self-test of the guard-band / poison-fill harness (tests/arena.py) on the CPU device, with torch ops standing in for the callee:
a clean callee passes, and every planted defect makes the harness fail with a message that names the buffer.  This is the evidence
that tests/test_gpu_buffer_contract.py can fail."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arena as A  # noqa: E402

N = 1000      # floats per buffer: 4000 bytes, not a multiple of the 256-byte alignment


def make():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, generator=g)
    acc = torch.randn(N, generator=g)
    return A.Arena([("x", x, "in"), ("y", N * 4, "out"), ("acc", acc, "inout"), ("ws", N * 4, "scratch")], "cpu"), x, acc


def clean(p):
    """y = 2x + 1 through the workspace (written before it is read), acc += x"""
    x, y, acc, ws = (p.view(n, torch.float32) for n in ("x", "y", "acc", "ws"))
    ws.copy_(x * 2)
    y.copy_(ws + 1)
    acc.add_(x)
    return 0


def test_layout_alignment_and_guards():
    ar, _, _ = make()
    p = ar.ptrs()
    assert A.GUARD == 64 * 1024 and A.FILLS == (0x00, 0xFF, 0x3C)
    ends = 0
    for name in ar.names:
        assert p[name] % 256 == 0, name
        assert ar.offset[name] - ends >= A.GUARD, name           # a full guard in front of every buffer
        ends = ar.offset[name] + ar.size[name]
    assert ar.total - ends == A.GUARD                             # and behind the last one
    covered = sum(b - a for a, b, _, _ in ar.guards) + sum(ar.size.values())
    assert covered == ar.total                                    # guards and buffers tile the arena: the guard starts at the next byte


def test_clean_callee_passes_and_returns_the_outputs():
    ar, x, acc = make()
    out = ar.check(clean)
    assert set(out) == {"y", "acc"}
    assert torch.equal(out["y"].view(torch.float32), x * 2 + 1)
    assert torch.equal(out["acc"].view(torch.float32), acc + x)


def guard_after(p):
    clean(p)
    p.arena[p.offset["y"] + p.size["y"]] = 1
    return 0


def guard_before(p):
    clean(p)
    p.arena[p.offset["y"] - 1] = 1
    return 0


def far_guard_byte(p):
    """the last byte of the guard in front of the first buffer's neighbour: every guard byte is looked at, not only the near ones"""
    clean(p)
    p.arena[p.offset["acc"] - 256] = 7
    return 0


def unwritten_byte(p):
    x, y, acc, ws = (p.view(n, torch.float32) for n in ("x", "y", "acc", "ws"))
    ws.copy_(x * 2)
    y.view(torch.uint8)[:-1].copy_((ws + 1).view(torch.uint8)[:-1])
    acc.add_(x)
    return 0


def stale_scratch_added(p):
    x, y, acc, ws = (p.view(n, torch.float32) for n in ("x", "y", "acc", "ws"))
    ws[1:].copy_(x[1:] * 2)                        # ws[0] keeps what it held on entry
    y.copy_(ws + 1)
    acc.add_(x)
    return 0


def stale_scratch_through_relu(p):
    x, y, acc, ws = (p.view(n, torch.float32) for n in ("x", "y", "acc", "ws"))
    stale = ws[0].clone()
    ws.copy_(x * 2)
    y.copy_(ws + 1)
    y[0] += torch.nan_to_num(stale.clamp(min=0), nan=0.0)      # max(0, stale) as the GPU's v_max does it: a NaN gives 0
    acc.add_(x)
    return 0


def modifies_input(p):
    clean(p)
    p.view("x")[17] ^= 1
    return 0


def inout_from_stale(p):
    x, y, acc, ws = (p.view(n, torch.float32) for n in ("x", "y", "acc", "ws"))
    ws.copy_(x * 2)
    acc.add_(y)                                    # reads the output before it is written
    y.copy_(ws + 1)
    return 0


PLANTED = [
    (guard_after, r"guard after 'y' \(bytes \+0\.\.\+0 past its end\)"),
    (guard_before, r"before 'y' \(bytes -1\.\.-1 from its start\)"),
    (far_guard_byte, r"guard after 'y' .* before 'acc' \(bytes -256\.\.-256 from its start\)"),
    (unwritten_byte, r"out buffer 'y' depends on the fill: 1 of 4000 byte\(s\).*first at \+3999.*1 of them still hold"),
    (stale_scratch_added, r"out buffer 'y' depends on the fill"),
    (stale_scratch_through_relu, r"out buffer 'y' depends on the fill.*0x00 and 0x3C"),
    (modifies_input, r"input 'x' modified.*first at \+17"),
    (inout_from_stale, r"inout buffer 'acc' depends on the fill"),
]


@pytest.mark.parametrize("callee,message", PLANTED, ids=[c.__name__ for c, _ in PLANTED])
def test_planted_defect_is_caught_and_names_the_buffer(callee, message):
    ar, _, _ = make()
    with pytest.raises(AssertionError, match=message):
        ar.check(callee)


def test_only_the_finite_fill_catches_a_stale_value_behind_relu():
    ar, _, _ = make()
    ar.check(stale_scratch_through_relu, fills=(0x00, 0xFF))          # a stale NaN is swallowed like a stale zero ...
    with pytest.raises(AssertionError, match="'y' depends on the fill"):
        ar.check(stale_scratch_through_relu, fills=(0x00, 0x3C))      # ... a stale 0.0115 is not


def test_return_code_is_asserted():
    ar, _, _ = make()
    with pytest.raises(AssertionError, match="return code -3"):
        ar.check(lambda p: clean(p) or -3)
    ar.run(0xFF, lambda p: -3, want_rc=-3, untouched=True)            # a refused call that touches nothing


def test_refused_call_must_leave_the_arena_unchanged():
    ar, _, _ = make()

    def refuses_late(p):
        p.view("ws")[5] = 9
        return -3
    with pytest.raises(AssertionError, match="refused call wrote 1 byte.*'ws'"):
        ar.run(0x00, refuses_late, want_rc=-3, untouched=True)


def test_declared_unwritten_output_must_keep_the_fill():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, generator=g)
    ar = A.Arena([("x", x, "in"), ("y", N * 4, "out"), ("unused", 64, "out")], "cpu")

    def callee(p):
        p.view("y", torch.float32).copy_(p.view("x", torch.float32))
        return 0
    ar.check(callee, unwritten=("unused",))
    with pytest.raises(AssertionError, match="'unused' depends on the fill"):
        ar.check(callee)                                             # not declared: an output nobody wrote

    def writes_it(p):
        p.view("unused")[3] = 1
        return callee(p)
    with pytest.raises(AssertionError, match="'unused' is declared unwritten"):
        ar.check(writes_it, unwritten=("unused",))
