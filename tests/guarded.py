"""Guard-banded operands for per-kernel tests (a plain helper module: import it, it is no conftest and defines no fixture).

An ``Arena`` lays every operand of ONE kernel call out in one flat allocation::

    | guard | operand 0 | guard | guard | operand 1 | guard | ...

and hands each operand to the kernel as ``ops.Sub(flat, offset)`` (``ops._p`` accepts a ``Sub`` for every pointer argument).  A stray
access of the kernel therefore lands in memory the test owns and shows up as an assertion of ``check()`` instead of a GPU fault.

Guard size.  Every operand has at least ``max(4096, 2 * ld)`` elements of guard before and after it (``ld`` = its row length, the last
dimension unless given); offsets are multiples of 4 elements, so 16-byte accesses keep their alignment.  The size is a CONDITION, not a
measurement: it must exceed one full row plus one 256-thread block of float4 (1024 elements), which is how far a kernel that mistakes a
row count, a column count or a block's share by one can reach.  A kernel that could reach further (a whole tile of rows, say) needs
``guard=`` on that operand.

Guard contents.
* Input operands are surrounded by NaN (integer arenas: by ``fill``, which the test chooses so that the kernel would turn it into a NaN
  or a wrong value).  An out-of-range read that reaches a result poisons it, and ``check()`` asserts that no output holds a NaN.
  WHAT THIS CANNOT SEE: a read whose value is masked off after the load (``v = p[i]; if (!ok) v = 0``, a product with an exact zero
  that the kernel forms with a select, a load into a register that is never used) leaves no trace; only the bounds of reads whose value
  reaches an output are tested.  Out-of-range WRITES are always seen.
* Output operands and their guards hold the sentinel bit pattern of the DPOT kernel tests (``-3.0e30``).
* In/out operands (``inout``: preloaded, then written -- the ``accumulate`` paths) hold the given tensor; their guards hold the sentinel.

``check()`` -- after the call and a synchronise -- asserts that
1. every guard, and every input operand, is bit-identical to what was written;
2. no output element still holds the sentinel, except the elements the test named (``unwritten=``: elements the kernel is documented not to
   write, e.g. the other columns of a column-range output) -- and those still hold exactly the sentinel;
3. no output element is a NaN;
4. for an in/out operand: its guards are intact and it holds no NaN (it was preloaded, so "never written" cannot be asked of it).

The arena works on CPU tensors as well; there ``Operand.op`` is the view itself, so that plain torch code can stand in for a kernel
(tests/test_unet_kernels_host.py proves with such fakes that each of the assertions above trips).
An arena has one dtype: fp32 by default, int32 for index tensors, fp64 for the fp64 output of rpb_reduce_partials (``ops.Sub`` counts
its offset in 4-byte elements, so an fp64 operand is handed over as ``Operand.tensor()``, the slice of the flat allocation)."""
import math

import torch

SENTINEL = -3.0e30
MIN_GUARD = 4096


def _up4(n):
    return (int(n) + 3) // 4 * 4


class Operand:
    def __init__(self, arena, name, kind, shape, ld, guard, data, unwritten):
        self.arena, self.name, self.kind, self.shape = arena, name, kind, tuple(int(s) for s in shape)
        self.n = math.prod(self.shape)
        self.ld = int(ld if ld is not None else (self.shape[-1] if self.shape else 1))
        self.guard = _up4(max(MIN_GUARD, 2 * self.ld, guard or 0))
        self.data, self.unwritten, self.off = data, unwritten, None

    @property
    def op(self):
        """what the kernel gets: ``ops.Sub(flat, offset)`` on a device, the (flat) view itself on the CPU"""
        return self.at(0)

    def at(self, offset):
        """the operand from element ``offset`` on (a column or row range of it; the leading dimension travels in the call)"""
        flat = self.arena._seal()
        if flat.device.type == "cpu":
            return flat[self.off + offset:self.off + self.n]
        from realpdebench_amd.ops import Sub
        return Sub(flat, self.off + offset)

    def tensor(self):
        """the operand as a 1-D slice of the flat allocation (for arguments that must be tensors, or whose elements are not 4 bytes)"""
        flat = self.arena._seal()
        return flat[self.off:self.off + self.n]

    def get(self):
        """the host copy of the operand after ``check()``"""
        assert self.arena._host is not None, "call Arena.check() first"
        return self.arena._host[self.off:self.off + self.n].view(self.shape).clone()


class Arena:
    def __init__(self, device, dtype=torch.float32, fill=None):
        """``fill``: the guard value around inputs (default NaN; an integer arena needs one)"""
        self.device, self.dtype = torch.device(device), dtype
        if fill is None:
            assert dtype.is_floating_point, "an integer arena needs a guard value"
            fill = float("nan")
        self.fill, self.items, self.flat, self.expect, self._host = fill, [], None, None, None

    # ------------------------------------------------------------------ operands
    def inp(self, t, name=None, ld=None, guard=None):
        """an input operand holding ``t`` (any shape; the kernel sees it row-major), NaN around it"""
        assert self.flat is None, "operands are declared before the first .op"
        o = Operand(self, name or f"in{len(self.items)}", "in", t.shape, ld, guard, t.detach().to("cpu", self.dtype).reshape(-1), None)
        self.items.append(o)
        return o

    def out(self, *shape, name=None, ld=None, guard=None, unwritten=None):
        """an output operand of ``shape``, sentinel inside and around.  ``unwritten``: bool tensor of ``shape``, True where the kernel is
        documented NOT to write"""
        assert self.flat is None, "operands are declared before the first .op"
        assert self.dtype.is_floating_point, "outputs are floating point (the sentinel is a float)"
        o = Operand(self, name or f"out{len(self.items)}", "out", shape, ld, guard, None, unwritten)
        if unwritten is not None:
            assert tuple(unwritten.shape) == o.shape and unwritten.dtype == torch.bool
        self.items.append(o)
        return o

    def inout(self, t, name=None, ld=None, guard=None):
        """an operand the kernel reads AND writes (``out += ...``): the body holds ``t``, the guards the sentinel, as for an output.
        ``check()`` asserts that the guards are intact and that the body holds no NaN.  It can make no never-written assertion, and
        needs none: a cell the kernel skips keeps its preloaded value, so its error against ``reference + t`` is the size of the
        result itself, which the max-error measure of the verdict catches (tests/test_mwt_kernels_host.py proves that with a fake)."""
        assert self.flat is None, "operands are declared before the first .op"
        assert self.dtype.is_floating_point, "in/out operands are floating point (the sentinel is a float)"
        o = Operand(self, name or f"inout{len(self.items)}", "inout", t.shape, ld, guard, t.detach().to("cpu", self.dtype).reshape(-1), None)
        self.items.append(o)
        return o

    def _seal(self):
        if self.flat is None:
            pos, spans = 0, []
            for o in self.items:
                pos += o.guard
                o.off = pos
                pos = _up4(pos + o.n) + o.guard
                spans.append(o)
            host = torch.empty(max(pos, 4), dtype=self.dtype)
            pos = 0
            for o in spans:                                        # guard | operand | (round-up) | guard, in the operand's own colour
                end = _up4(o.off + o.n) + o.guard
                host[pos:end] = self.fill if o.kind == "in" else SENTINEL
                if o.kind != "out":
                    host[o.off:o.off + o.n] = o.data
                    o.data = None
                pos = end
            self.expect = host
            self.flat = host.clone() if self.device.type == "cpu" else host.to(self.device)
        return self.flat

    # ------------------------------------------------------------------ the three assertions
    @staticmethod
    def _bits(t):
        return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))

    def check(self):
        flat = self._seal()
        if flat.device.type != "cpu":
            torch.cuda.synchronize()
        self._host = h = flat.cpu() if flat.device.type != "cpu" else flat.clone()
        hb, eb = self._bits(h), self._bits(self.expect)
        pos = 0
        for o in self.items:
            end = _up4(o.off + o.n) + o.guard
            for what, lo, hi in (("before", pos, o.off), ("after", o.off + o.n, end)):
                bad = (hb[lo:hi] != eb[lo:hi]).nonzero()
                if bad.numel():
                    i = int(bad[0]) + lo
                    dist = (o.off - i) if what == "before" else (i - (o.off + o.n) + 1)
                    raise AssertionError(f"guard {what} operand '{o.name}' {o.shape} was written: {bad.numel()} element(s), the first "
                                         f"{dist} element(s) {what} it (value {float(h[i])!r})")
            body, ebody = hb[o.off:o.off + o.n], eb[o.off:o.off + o.n]
            if o.kind == "in":
                bad = (body != ebody).nonzero()
                assert not bad.numel(), (f"input operand '{o.name}' {o.shape} was written: {bad.numel()} element(s), the first at flat "
                                         f"index {int(bad[0])}")
            elif o.kind == "inout":
                nan = torch.isnan(h[o.off:o.off + o.n]).nonzero()
                assert not nan.numel(), (f"in/out operand '{o.name}' {o.shape}: {nan.numel()} NaN(s) -- a read outside an input operand "
                                         f"reached the result (first at flat index {int(nan[0])})")
            else:
                val = h[o.off:o.off + o.n]
                still = body == ebody                               # the interior started as all-sentinel
                if o.unwritten is not None:
                    named = o.unwritten.reshape(-1)
                    wrote = (~still & named).nonzero()
                    assert not wrote.numel(), (f"output '{o.name}' {o.shape}: {wrote.numel()} element(s) the kernel is documented not "
                                               f"to write were written, the first at flat index {int(wrote[0])}")
                    still, val = still & ~named, val[~named]
                left = still.nonzero()
                assert not left.numel(), (f"output '{o.name}' {o.shape}: {left.numel()} element(s) were never written, the first at flat "
                                          f"index {int(left[0])}")
                nan = torch.isnan(val).nonzero()
                assert not nan.numel(), (f"output '{o.name}' {o.shape}: {nan.numel()} NaN(s) -- a read outside an input operand reached "
                                         f"the result (first at {int(nan[0])} of the written elements)")
            pos = end
        return self
