"""Guard-band / poison-fill harness for the C ABI's buffer contract (a plain helper module, imported by tests/test_cpu_arena.py
and tests/test_gpu_buffer_contract.py).

Every buffer a call gets is carved out of ONE allocation, 256-byte aligned, with a guard band in front of it and one immediately
behind its last byte.  The whole allocation is filled with one byte value before the call, so

  * a write outside [ptr, ptr + bytes) of any argument shows as a guard byte that is no longer the fill,
  * a modified `const` argument shows as an `in` buffer that differs from what was copied in,
  * an output byte nobody wrote, or an output that depends on what the workspace / the output held on entry, shows as an output
    that differs between two fills.

The fills: 0x00 (hides nothing 0x3C does not reveal, but 0x00 against 0xFF proves that every output byte is written), 0xFF (fp16 and
fp32 NaN, counters at -1, labels 255) and 0x3C (finite positive: fp16 1.06, fp32 0.0115 -- ReLU, max and comparisons swallow a stale
NaN exactly as they would a stale zero, a stale 1.06 they do not).

What the method cannot see: out-of-range READS whose values never reach an output, and overruns that jump over a whole guard into
the middle of a scratch buffer.
"""
import torch

# Guard width.  A condition, not a measurement: it has to be wider than one 16-row tile strip of the widest activation the GPU cases
# use, so that a kernel that runs one strip past (or before) a tensor lands in a guard.  Activations are fp16 NHWC with the channel
# count padded to a multiple of 8, and a level's row has the same bytes as the level above (half the pixels, twice the channels).
# Widest rows of the small cases: 80 pixels x 24 channels x 2 B (48 x 80, alpha 1.25: 20 channels padded to 24) = 3840 B, a strip
# 16 x 3840 = 61440 B = 60 KiB < 64 KiB; the others are narrower (32 x 48, alpha 2: 48 KiB; EvalNet 'city', 208 x 8 channels: 52 KiB).
# Two kinds of tensor are wider and NOT covered by the guard alone: the many-tiles cases' rows (256 pixels x 8 channels x 2 B =
# 4096 B, a strip exactly 64 KiB), and the 35-class tensors (fp16 logits / one-hot input 40 channels, fp32 probabilities: 100 to
# 260 KiB per strip).  A whole-strip overrun of those, like every overrun larger than the guard, ends in the neighbouring buffer
# and has to be caught by the input-unchanged and output-equality checks, so the GPU tests never put the exempt workspace behind
# another buffer.
GUARD = 64 * 1024
ALIGN = 256
FILLS = (0x00, 0xFF, 0x3C)
ROLES = ("in", "out", "inout", "scratch")


def _align(n, a=ALIGN):
    return (n + a - 1) // a * a


def as_bytes(t):
    """a tensor of any dtype as a flat uint8 tensor (a copy if it is not contiguous)"""
    return t.contiguous().reshape(-1).view(torch.uint8)


class Ptrs(dict):
    """name -> address of the buffer's first byte; `arena` / `offset` for callees that work on the tensor itself (the CPU self-test)"""

    def __init__(self, arena, offset, size):
        super().__init__({n: arena.data_ptr() + o for n, o in offset.items()})
        self.arena, self.offset, self.size = arena, offset, size

    def view(self, name, dtype=torch.uint8):
        o = self.offset[name]
        return self.arena[o:o + self.size[name]].view(dtype)


class Arena:
    """specs: a list of (name, nbytes, role) or (name, tensor, role); a tensor gives size and, for `in` / `inout`, the content"""

    def __init__(self, specs, device, guard=GUARD):
        self.device = torch.device(device)
        self.guard = guard
        self.names, self.role, self.size, self.offset, self.content = [], {}, {}, {}, {}
        pos = guard
        for name, what, role in specs:
            assert role in ROLES, role
            assert name not in self.role, f"buffer {name!r} listed twice"
            if torch.is_tensor(what):
                data = as_bytes(what)
                nbytes = data.numel()
            else:
                data, nbytes = None, int(what)
            assert nbytes > 0, f"buffer {name!r} is empty"
            if role in ("in", "inout"):
                assert data is not None, f"{role} buffer {name!r} needs its content"
                self.content[name] = data.to(self.device)
            pos = _align(pos)
            self.names.append(name)
            self.role[name], self.size[name], self.offset[name] = role, nbytes, pos
            pos += nbytes + guard                     # the guard starts at the byte right behind the buffer
        self.total = pos
        raw = torch.empty(self.total + ALIGN, dtype=torch.uint8, device=self.device)
        skip = (-raw.data_ptr()) % ALIGN
        self.mem = raw[skip:skip + self.total]
        # the guards: the gaps between consecutive buffers and the two ends, (first byte, end, buffer in front or None, buffer behind or None)
        self.guards = []
        end, prev = 0, None
        for name in self.names:
            self.guards.append((end, self.offset[name], prev, name))
            end, prev = self.offset[name] + self.size[name], name
        self.guards.append((end, self.total, prev, None))

    def view(self, name, dtype=torch.uint8):
        o = self.offset[name]
        return self.mem[o:o + self.size[name]].view(dtype)

    def ptrs(self):
        return Ptrs(self.mem, self.offset, self.size)

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()

    def _check_guards(self, fill):
        bad = torch.stack([(self.mem[a:b] != fill).sum() for a, b, _, _ in self.guards]).cpu()
        for (a, b, prev, nxt), n in zip(self.guards, bad.tolist()):
            if n:
                idx = torch.nonzero(self.mem[a:b] != fill)[:, 0]
                first, last = a + int(idx[0]), a + int(idx[-1])
                where = []
                if prev is not None:
                    where.append(f"after {prev!r} (bytes +{first - a}..+{last - a} past its end)")
                if nxt is not None:
                    where.append(f"before {nxt!r} (bytes -{b - first}..-{b - last} from its start)")
                raise AssertionError(f"guard {' / '.join(where)} written: {n} byte(s) differ from fill 0x{fill:02X}")

    def run(self, fill, call, want_rc=0, untouched=False):
        """fill the arena, put the inputs in place, call, synchronise; assert guards, inputs and the return code; return the snapshots
        {name: uint8 tensor} of every out / inout buffer.  untouched: the call has to leave the WHOLE arena as it was (a refused call)."""
        self.mem.fill_(fill)
        for name, data in self.content.items():
            self.view(name).copy_(data)
        before = self.mem.clone() if untouched else None
        self._sync()
        rc = call(self.ptrs())
        self._sync()
        assert rc == want_rc, f"return code {rc} (want {want_rc}) with fill 0x{fill:02X}"       # (c)
        self._check_guards(fill)                                                                   # (a)
        for name in self.names:                                                                    # (b)
            if self.role[name] == "in" and not torch.equal(self.view(name), self.content[name]):
                d = torch.nonzero(self.view(name) != self.content[name])[:, 0]
                raise AssertionError(f"input {name!r} modified with fill 0x{fill:02X}: {d.numel()} byte(s), first at +{int(d[0])}")
        if untouched:
            d = torch.nonzero(self.mem != before)[:, 0]
            if d.numel():
                at = int(d[0])
                name = [n for n in self.names if self.offset[n] <= at][-1:] or self.names[:1]
                raise AssertionError(f"a refused call wrote {d.numel()} byte(s), first at arena byte {at} (in or after {name[0]!r})")
        return {n: self.view(n).clone() for n in self.names if self.role[n] in ("out", "inout")}

    def check(self, call, unwritten=(), fills=FILLS, ranges=None):
        """run with every fill; every out / inout buffer has to be byte-identical across the fills, except the ones in `unwritten`
        (declared not written on this route), which have to be all fill.  ranges: {name: (first byte, end)} for a buffer of which the
        header declares only that part a result (the rest is scratch or reserved); the snapshots are cut to it.
        Returns the snapshots of the first fill (0x00)."""
        snaps = {f: self.run(f, call) for f in fills}
        for name, (lo, hi) in (ranges or {}).items():
            assert self.role[name] in ("out", "inout") and 0 <= lo < hi <= self.size[name], name
            for f in fills:
                snaps[f][name] = snaps[f][name][lo:hi]
        first = snaps[fills[0]]
        for name in first:
            if name in unwritten:
                for f in fills:
                    n = int((snaps[f][name] != f).sum())
                    assert n == 0, f"output {name!r} is declared unwritten but {n} byte(s) differ from fill 0x{f:02X}"
                continue
            for f in fills[1:]:
                if not torch.equal(first[name], snaps[f][name]):
                    d = torch.nonzero(first[name] != snaps[f][name])[:, 0]
                    stale = int((snaps[f][name][d] == f).sum())
                    raise AssertionError(
                        f"{self.role[name]} buffer {name!r} depends on the fill: {d.numel()} of {first[name].numel()} byte(s) differ between "
                        f"fill 0x{fills[0]:02X} and 0x{f:02X}, first at +{int(d[0])}, last at +{int(d[-1])}; {stale} of them still hold "
                        f"the fill (unwritten), the others come from a stale value")
        return first
