"""Guard-band harness for the C ABI (include/xmlhip.h): every operand, output and workspace of one call is carved out of
ONE byte arena filled with a known byte, so that a store outside a documented extent, a read of bytes nobody defined and a
workspace formula that is too small all become visible.  A plain helper module (tests/test_abi_arena.py checks it on the
CPU with fake cases, tests/test_gpu_abi_arena.py runs the real entries through it).

A case runs twice, on a fresh 0x00 arena and on a fresh 0xFF arena (NaN in f32 / bf16 / f16, -1 in int32 / int64, all bits
set in a bit word): a stray store of zeros shows under 0xFF, any other stray store under 0x00, and a read of outside bytes
that reaches a result changes the result between the two.
"""
import ctypes

import torch

MARGIN = 1 << 20          # untouched bytes at both ends of an arena
FILLS = (0x00, 0xFF)


class ArenaError(AssertionError):
    pass


class Region(object):
    """One carved operand: `view` is the typed (possibly row-strided) tensor; its bytes are [off, end) of the arena, of
    which only the bytes of the rows themselves are owned -- the bytes between strided rows stay guard bytes."""

    def __init__(self, name, off, end, view, row_bytes, ld_bytes, n_rows, written_mask=None):
        self.name, self.off, self.end, self.view = name, off, end, view
        self.row_bytes, self.ld_bytes, self.n_rows = row_bytes, ld_bytes, n_rows
        self.written_mask = written_mask       # bool, view's shape: the elements the header defines (None: all of them)
        self.source = None                     # CPU tensor copied in by put(): an operand the entry must not change
        self.may_mask = None                   # bool: undefined elements that the entry may nevertheless write


def _bits(t):
    """contiguous byte image of a tensor (bitwise comparisons: NaN == NaN, -0 != +0)."""
    t = t.contiguous()
    return t.view(-1).view(torch.uint8) if t.numel() else t.view(-1).to(torch.uint8)


class Arena(object):
    def __init__(self, nbytes, fill, device):
        assert fill in (0x00, 0xFF) or 0 <= fill < 256
        self.fill, self.device = int(fill), torch.device(device)
        self.size = MARGIN + int(nbytes) + MARGIN
        self.buf = torch.full((self.size,), self.fill, dtype=torch.uint8, device=self.device)
        self.owned = torch.zeros((self.size,), dtype=torch.bool, device=self.device)
        self.base = self.buf.data_ptr()
        self.cursor = MARGIN
        self.regions = []

    # ---- carving ----
    def take(self, name, shape, dtype, align=256, gap=4096, ld=None, skew=0, partly_written=None, may_be_written=None):
        """A region of `shape` / `dtype` whose first byte lies `skew` bytes past an `align`-aligned ADDRESS, with at least
        `gap` untouched bytes on each side.  ld (elements): row stride of the last dimension, >= shape[-1]; the leading
        dimensions are flattened into rows.  partly_written: bool mask (shape) of the elements the entry defines; the others
        must still hold the fill afterwards -- except those of may_be_written (bool mask), which the header neither defines
        nor promises to leave alone (padding of a 16-byte piece, a trailer's spare bytes).  The region is exactly the documented extent: (rows - 1) * ld + n elements."""
        shape = tuple(int(s) for s in shape)
        es = torch.empty(0, dtype=dtype).element_size()
        n = shape[-1] if shape else 1
        rows = 1
        for s in shape[:-1]:
            rows *= s
        ld = n if ld is None else int(ld)
        assert ld >= n and skew % es == 0 and align % es == 0
        numel = ((rows - 1) * ld + n) if rows > 0 and n > 0 else 0
        addr = self.base + self.cursor + gap
        addr = (addr + align - 1) // align * align + skew
        off = addr - self.base
        end = off + numel * es
        if end + gap > self.size - MARGIN:
            raise ArenaError("arena too small for region %r (%d bytes needed)" % (name, end + gap + MARGIN - self.size))
        flat = self.buf[off:end].view(dtype) if numel else torch.empty(0, dtype=dtype, device=self.device)
        if numel:
            strides, acc = [], ld
            for s in reversed(shape[:-1]):
                strides.append(acc)
                acc *= s
            view = flat.as_strided(shape, tuple(reversed(strides)) + (1,))
            own = self.owned[off:end]
            if ld == n:
                own.fill_(True)
            else:
                own.as_strided((rows, n * es), (ld * es, 1)).fill_(True)
        else:
            view = flat.view(shape)
        if partly_written is not None:
            partly_written = torch.as_tensor(partly_written, dtype=torch.bool).to(self.device)
            assert tuple(partly_written.shape) == shape
        reg = Region(name, off, end, view, n * es, ld * es, rows, partly_written)
        if may_be_written is not None:
            reg.may_mask = torch.as_tensor(may_be_written, dtype=torch.bool).to(self.device)
            assert tuple(reg.may_mask.shape) == shape and partly_written is not None
        assert all(r.name != name for r in self.regions), "region %r taken twice" % name
        self.regions.append(reg)
        self.cursor = end
        return view

    def put(self, name, cpu_tensor, **kw):
        """take + copy-in: an input operand.  check_inputs() later asserts the entry left it alone."""
        v = self.take(name, cpu_tensor.shape, cpu_tensor.dtype, **kw)
        v.copy_(cpu_tensor)
        self.regions[-1].source = cpu_tensor.clone()
        return v

    def workspace(self, nbytes, name="ws"):
        """scratch of EXACTLY nbytes (what the matching *_workspace_bytes() returned) -> (pointer, nbytes)."""
        nbytes = int(nbytes)
        v = self.take(name, (nbytes,), torch.uint8)
        return (ctypes.c_void_p(v.data_ptr()) if nbytes else None), nbytes

    def region(self, name):
        for r in self.regions:
            if r.name == name:
                return r
        raise KeyError(name)

    # ---- checks ----
    def _describe(self, pos):
        best = None
        for r in self.regions:
            if r.off <= pos < r.end:
                row, col = divmod(pos - r.off, r.ld_bytes)
                return "inside region %r, in the gap behind row %d (%d bytes past the row's last byte)" % (
                    r.name, row, col - r.row_bytes + 1)
            d, side = (r.off - pos, "before the start") if pos < r.off else (pos - r.end + 1, "after the end")
            if best is None or d < best[0]:
                best = (d, side, r.name)
        if best is None:
            return "no region recorded"
        return "%d bytes %s of region %r" % best

    def check_guards(self):
        """Every byte outside the recorded regions (the gaps between strided rows included) still equals the fill.
        Computed on the device: one flag comes back, and on failure the offset of the first changed byte."""
        bad = (self.buf != self.fill) & ~self.owned
        n_bad = int(bad.sum())
        if n_bad:
            pos = int(torch.nonzero(bad)[0])
            raise ArenaError("fill 0x%02X: %d guard bytes changed; the first at arena offset %d holds 0x%02X: %s"
                             % (self.fill, n_bad, pos, int(self.buf[pos]), self._describe(pos)))

    def check_inputs(self):
        for r in self.regions:
            if r.source is not None and not torch.equal(_bits(r.view.cpu()), _bits(r.source)):
                raise ArenaError("fill 0x%02X: the entry changed its input operand, region %r" % (self.fill, r.name))

    def region_of(self, view):
        for r in self.regions:
            if r.view.data_ptr() == view.data_ptr() and r.view.shape == view.shape:
                return r
        raise ArenaError("an output view that is no region of the arena")


def ptr(t, byte_offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_offset)


class Case(object):
    """One guard-band case.
      symbols  the header entries the case is about (the completeness test counts them)
      inputs   () -> dict of CPU tensors / Python values, deterministic
      raw      (lib, arena, inp) -> (status or list of statuses, dict name -> output view in the arena)
      wrapper  (inp moved to the device) -> dict name -> tensor: the tested ops.* path on ordinary contiguous tensors
      nbytes   payload bytes the arena needs (regions + gaps)
      atomic   None, or tol: the entry accumulates with atomics (order dependent): outputs are finite under 0xFF and agree
               with the wrapper within max|got - want| <= tol * max|want|, the measure and bound of the entry's existing test
      note     which tail the shape hits"""


    def __init__(self, name, symbols, inputs, raw, wrapper, nbytes=1 << 20, atomic=None, note="", canon=None, expect_status=0):
        self.name, self.symbols, self.inputs, self.raw, self.wrapper = name, tuple(symbols), inputs, raw, wrapper
        self.nbytes, self.atomic, self.note = int(nbytes), atomic, note
        # canon: output name -> f(tensor, defined mask) -> tensor, for an output whose header leaves the ORDER of its
        # entries unspecified (applied to both runs and to the wrapper's result before they are compared)
        self.canon = canon or {}
        # expect_status != 0: a documented refusal -- the entry returns that status and writes nothing at all
        self.expect_status = int(expect_status)

    def __repr__(self):
        return self.name


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _to_device(inp, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}


def run_case(case, lib, device):
    """Run `case` under both fills and assert, in this order: status, guards (and untouched inputs), fill independence,
    same values as the wrapper."""
    inp = case.inputs()
    runs = []
    for fill in FILLS:
        arena = Arena(case.nbytes, fill, device)
        status, outs = case.raw(lib, arena, inp)
        _sync(device)
        runs.append((arena, status, outs))
    # 1. status
    for arena, status, _ in runs:
        for s in (status if isinstance(status, (list, tuple)) else [status]):
            if s != case.expect_status:
                raise ArenaError("%s, fill 0x%02X: the entry returned status %d" % (case.name, arena.fill, s))
    # 2. guards
    for arena, _, _ in runs:
        try:
            arena.check_guards()
            arena.check_inputs()
        except ArenaError as e:
            raise ArenaError("%s: %s" % (case.name, e))
    (a0, _, o0), (a1, _, o1) = runs
    if case.expect_status != 0:          # a refusal comes before any launch: every output still holds the fill
        for arena, _, outs in runs:
            for name, v in outs.items():
                if bool((_bits(arena.region_of(v).view.cpu()) != arena.fill).any()):
                    raise ArenaError("%s, fill 0x%02X: the entry refused the call but wrote to output %r" % (case.name, arena.fill, name))
        return {}
    # 3. fill independence
    assert sorted(o0) == sorted(o1)
    host = {}
    for name in sorted(o0):
        r0, r1 = a0.region_of(o0[name]), a1.region_of(o1[name])
        v0, v1 = r0.view.cpu(), r1.view.cpu()
        mask = None if r0.written_mask is None else r0.written_mask.cpu()
        if mask is not None:
            for v, fill, reg in ((v0, 0x00, r0), (v1, 0xFF, r1)):
                touched = (_bits(v) != fill).view(-1, v.element_size()).any(1).view(v.shape) & ~mask
                if reg.may_mask is not None:
                    touched &= ~reg.may_mask.cpu()
                if bool(touched.any()):
                    raise ArenaError("%s: output %r (region %r), fill 0x%02X: %d elements the header declares unwritten were "
                                     "written; the first at index %s" % (case.name, name, reg.name, fill, int(touched.sum()),
                                                                         [int(i) for i in torch.nonzero(touched)[0]]))
        if name in case.canon:
            v0, v1 = case.canon[name](v0, mask), case.canon[name](v1, mask)
        if case.atomic is not None:
            if v1.is_floating_point() and not bool(torch.isfinite(v1.float()).all()):
                raise ArenaError("%s: output %r (region %r) holds NaN / Inf under fill 0xFF" % (case.name, name, r1.name))
        else:
            es = v0.element_size()
            d = (_bits(v0) != _bits(v1)).view(-1, es).any(1).view(v0.shape)
            if mask is not None:
                d = d & mask
            if bool(d.any()):
                first = [int(i) for i in torch.nonzero(d)[0]]
                both = ("the fill in both runs: never written" if bool((_bits(v0[tuple(first)]) == 0x00).all()) and
                        bool((_bits(v1[tuple(first)]) == 0xFF).all()) else "a value that depends on the fill")
                raise ArenaError("%s: output %r (region %r): %d defined elements differ between the 0x00 and the 0xFF run; "
                                 "the first, at index %s, holds %s" % (case.name, name, r0.name, int(d.sum()), first, both))
        host[name] = (v0, v1, mask, r0.name)
    # 4. the same values as the tested path
    if case.wrapper is not None:
        want = case.wrapper(_to_device(inp, device))
        _sync(device)
        assert sorted(want) == sorted(host), (sorted(want), sorted(host))
        for name, (v0, v1, mask, rname) in host.items():
            w = want[name].cpu()
            if name in case.canon:
                w = case.canon[name](w, mask)
            assert tuple(w.shape) == tuple(v0.shape) and w.dtype == v0.dtype, \
                "%s: output %r: wrapper gives %s %s, the case %s %s" % (case.name, name, tuple(w.shape), w.dtype,
                                                                        tuple(v0.shape), v0.dtype)
            if case.atomic is not None:
                for v in (v0, v1):
                    err = float((v.double() - w.double()).abs().max() / w.double().abs().max().clamp_min(1e-30))
                    if not err <= case.atomic:
                        raise ArenaError("%s: output %r (region %r): max err / max|wrapper| = %.3e > %.1e" % (
                            case.name, name, rname, err, case.atomic))
                continue
            d = (_bits(v0) != _bits(w)).view(-1, v0.element_size()).any(1).view(v0.shape)
            if mask is not None:
                d = d & mask
            if bool(d.any()):
                first = tuple(int(i) for i in torch.nonzero(d)[0])
                raise ArenaError("%s: output %r (region %r): %d elements differ bitwise from the wrapper's; the first at index "
                                 "%s: %r against %r" % (case.name, name, rname, int(d.sum()), list(first), v0[first].item(),
                                                        w[first].item()))
    return host
