"""A guarded, poisoned arena for the buffers a kernel writes, reads or borrows (plain torch, any device).

The value tests compare what a kernel computed; this module checks WHERE it read and wrote.  An `Arena` is one
`torch.empty(nbytes, dtype=uint8)` block.  Tensors are carved from it as views at 256-byte-aligned offsets (what torch's
allocator gives and the strictest alignment include/mvs_abi.h asks for), each between two guard bands filled with
GUARD.  Every carved tensor has a role:

  in       the kernel may only read it: `check()` reports any changed byte;
  out      the kernel must write every element: the payload is filled with the poison byte before the call;
  scratch  a workspace the kernel borrows: poisoned like `out`, so a read of bytes nobody wrote shows in the outputs;
  inout    read and updated in place (running statistics, a running accumulator): never poisoned, only guarded.

Guard width: the bytes of one slice of the tensor's outermost dimension (for a [D, h, w] volume one z-plane), at least
MIN_GUARD = 64 KiB, rounded up to the alignment.  An off-by-one in x, y or z lands within one plane of either end, so
that width is derived from the indexing, not measured.  The guard behind a tensor starts at the byte after its last
element (a workspace of exactly the queried size has its guard directly behind it).

The three poisons, and what each is for:
  0x00  what fresh memory looks like (the value a missed write usually meets, so it alone finds nothing);
  0xFF  NaN as fp32, fp16, bf16 and fp64, -1 as int32: an unwritten element, or a scratch read that reaches an output
        even behind a zero factor (0 * NaN = NaN), shows as NaN;
  0x4B  finite and large (1.3e7 as fp32 / bf16, 14.6 as fp16): against 0x00 it shows a scratch read that a finite
        check would let through.
`same_under_all_poisons` runs a call once per poison on the same inputs and asserts that the outputs are the same
bytes in all three runs, that no guard byte changed and that no `in` tensor changed.
"""
import contextlib

import torch

ALIGN = 256
MIN_GUARD = 64 << 10
GUARD = 0xA5
POISONS = (0x00, 0xFF, 0x4B)
ROLES = ("in", "out", "scratch", "inout")


def _round_up(n, a):
    return (n + a - 1) // a * a


class Carved:
    """One tensor of the arena: `tensor` (the view), its role, and the byte ranges [lo, start) and [end, hi) of its
    guards inside the arena's block."""

    def __init__(self, name, role, tensor, lo, start, end, hi):
        self.name, self.role, self.tensor = name, role, tensor
        self.lo, self.start, self.end, self.hi = lo, start, end, hi
        self.snapshot = None

    @property
    def guard_bytes(self):
        return (self.start - self.lo) + (self.hi - self.end)


class Arena:
    def __init__(self, nbytes, device="cpu"):
        self.device = torch.device(device)
        self.block = torch.empty(nbytes + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = (-self.block.data_ptr()) % ALIGN      # first 256-byte-aligned byte of the block
        self.poison = POISONS[0]
        self.reset()

    # ---------------------------------------------------------------- carving
    def reset(self, poison=None):
        """Forget every carved tensor (the block is kept); later `out` / `scratch` tensors get `poison`."""
        if poison is not None:
            if poison not in POISONS:
                raise ValueError(f"poison must be one of {POISONS}")
            self.poison = poison
        self.cursor = self.base
        self.carved = []

    def carve(self, shape, dtype, role, name=None, guard=None):
        """A contiguous tensor of `shape` and `dtype` between two guards; `out` and `scratch` are poisoned."""
        if role not in ROLES:
            raise ValueError(f"role must be one of {ROLES}, got {role!r}")
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * item
        slice_bytes = nbytes // shape[0] if shape and shape[0] else nbytes
        width = _round_up(max(MIN_GUARD, slice_bytes, guard or 0), ALIGN)
        lo = self.cursor
        start = lo + width
        end = start + nbytes
        hi = self.base + _round_up(end + width - self.base, ALIGN)
        if hi > self.block.numel():
            raise MemoryError(f"arena of {self.block.numel()} bytes is full: {name or role} needs bytes up to {hi}")
        self.cursor = hi
        self.block[lo:start].fill_(GUARD)
        self.block[end:hi].fill_(GUARD)
        t = self.block[start:end].view(dtype).view(shape)
        assert t.data_ptr() % ALIGN == 0
        rec = Carved(name or f"{role}{len(self.carved)}", role, t, lo, start, end, hi)
        self.carved.append(rec)
        if role in ("out", "scratch"):
            self.poison_one(rec)
        return t

    def put(self, src, role="in", name=None):
        """A copy of `src` in the arena; an `in` tensor's bytes are remembered for `check()`."""
        if role not in ("in", "inout"):
            raise ValueError("put() places data: role 'in' or 'inout'")
        t = self.carve(src.shape, src.dtype, role, name)
        t.copy_(src)
        rec = self.carved[-1]
        if role == "in":
            rec.snapshot = self.block[rec.start:rec.end].clone()
        return t

    def record(self, t):
        for rec in self.carved:
            if rec.tensor is t or (rec.tensor.data_ptr() == t.data_ptr() and rec.tensor.shape == t.shape
                                   and rec.tensor.dtype == t.dtype):
                return rec
        raise KeyError("tensor was not carved from this arena")

    def owner(self, t):
        """The carved tensor whose payload holds every byte of `t` (a carved tensor or a view of one), else KeyError:
        `t` is an ordinary allocation, neither poisoned nor guarded."""
        if t.device == self.block.device and t.numel():
            a = t.data_ptr() - self.block.data_ptr()
            b = a + ((sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1) * t.element_size())
            for rec in self.carved:
                if rec.start <= a and b <= rec.end:
                    return rec
        raise KeyError("tensor does not lie in a payload of this arena")

    def poison_one(self, rec, poison=None):
        """Fill one payload with the poison byte.  Refused for `in` and `inout`: their bytes are data."""
        if not isinstance(rec, Carved):
            rec = self.record(rec)
        if rec.role not in ("out", "scratch"):
            raise ValueError(f"{rec.name} has role {rec.role!r}: only 'out' and 'scratch' buffers may be poisoned")
        self.block[rec.start:rec.end].fill_(self.poison if poison is None else poison)

    # ---------------------------------------------------------------- checking
    @property
    def guard_bytes(self):
        return sum(r.guard_bytes for r in self.carved)

    def check(self):
        """After the call (and one synchronise): a list of findings, empty when every guard byte still holds GUARD and
        every `in` tensor its bytes."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        out = []
        for r in self.carved:
            for side, a, b in (("before", r.lo, r.start), ("after", r.end, r.hi)):
                bad = self.block[a:b] != GUARD
                if bool(bad.any()):
                    first = int(torch.nonzero(bad)[0])
                    off = first - (r.start - a) if side == "before" else first
                    out.append(f"guard {side} {r.name} ({r.role}, {tuple(r.tensor.shape)} {r.tensor.dtype}): "
                               f"{int(bad.sum())} bytes changed, first at offset {off} from the "
                               f"{'start' if side == 'before' else 'end'} of the tensor")
            if r.role == "in" and r.snapshot is not None:
                bad = self.block[r.start:r.end] != r.snapshot
                if bool(bad.any()):
                    out.append(f"input {r.name} ({tuple(r.tensor.shape)} {r.tensor.dtype}) was modified: "
                               f"{int(bad.sum())} bytes changed, first at byte {int(torch.nonzero(bad)[0])}")
        return out

    # ---------------------------------------------------------------- running library wrappers inside the arena
    @contextlib.contextmanager
    def intercept(self, module):
        """While active, the name `torch` in `module` is a proxy whose `empty` / `empty_like` carve from this arena
        (tensors on the arena's device only; a 1-D uint8 tensor is a workspace: `scratch`, everything else `out`)
        and record what they gave out; everything else is torch's own.  The module's code is not changed.  An allocation
        on the arena's device that the proxy cannot carve (another allocation function, extra keywords, a
        non-contiguous `empty_like`) fails the block on exit."""
        real = module.torch
        proxy = module.torch = _TorchProxy(real, self)
        try:
            yield self
        finally:
            module.torch = real
        # reached only when the body raised nothing: an allocation on the arena's device that the proxy could not carve
        # would be an unpoisoned, unguarded buffer in a case that still passes
        assert not proxy.uncarved, f"{module.__name__} allocated outside the arena: {proxy.uncarved}"


class _TorchProxy:
    OTHER_ALLOCATORS = ("zeros", "ones", "full", "empty_strided", "zeros_like", "ones_like", "full_like", "rand", "randn",
                        "rand_like", "randn_like", "tensor", "as_tensor", "arange")

    def __init__(self, real, arena):
        self._real, self._arena = real, arena
        self.uncarved = []

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if name not in self.OTHER_ALLOCATORS:
            return f

        def watched(*a, **kw):
            t = f(*a, **kw)
            if self._mine(t.device):
                self.uncarved.append(f"torch.{name} -> {tuple(t.shape)} {t.dtype}")
            return t
        return watched

    def _mine(self, device):
        if device is None:
            return self._arena.device.type == "cpu"
        d = self._real.device(device)
        a = self._arena.device
        return d.type == a.type and (d.index is None or a.index is None or d.index == a.index)

    def empty(self, *size, dtype=None, device=None, **kw):
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        dtype = dtype or self._real.get_default_dtype()
        if kw or not self._mine(device):
            if self._mine(device):
                self.uncarved.append(f"torch.empty{size} with {sorted(kw)}")
            return self._real.empty(size, dtype=dtype, device=device, **kw)
        role = "scratch" if dtype == self._real.uint8 and len(size) == 1 else "out"
        return self._arena.carve(size, dtype, role)

    def empty_like(self, t, **kw):
        if kw or not t.is_contiguous():
            if self._mine(t.device):
                self.uncarved.append(f"torch.empty_like({tuple(t.shape)}, strides {t.stride()}) with {sorted(kw)}")
            return self._real.empty_like(t, **kw)
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)


def raw_bytes(t):
    """A host copy of a tensor's bytes (NaN payloads and signed zeros included)."""
    return t.detach().contiguous().reshape(-1).view(torch.uint8).to("cpu", copy=True)


def same_under_all_poisons(arena, fn):
    """Runs `fn(arena)` once per poison: `fn` places its inputs with `arena.put`, carves (or lets an intercepted
    wrapper carve) its outputs and workspaces, calls the kernel and returns the output tensor or a tuple of them.
    After each run the guards and inputs are checked.  Asserts the outputs are bit-identical across the three runs and
    returns (the outputs' bytes as host tensors, guard bytes checked per run)."""
    runs, guard_bytes = [], 0
    for p in POISONS:
        arena.reset(poison=p)
        outs = fn(arena)
        if isinstance(outs, torch.Tensor):
            outs = (outs,)
        outs = tuple(o for o in outs if o is not None)
        for k, o in enumerate(outs):      # an output outside the arena would be compared unpoisoned and unguarded
            try:
                role = arena.owner(o).role
            except KeyError:
                raise AssertionError(f"output {k} ({tuple(o.shape)} {o.dtype}) was not carved from the arena") from None
            assert role in ("out", "inout"), f"output {k} lies in a tensor of role {role!r}"
        findings = arena.check()
        assert not findings, f"poison 0x{p:02X}: " + "; ".join(findings)
        guard_bytes = arena.guard_bytes
        runs.append([raw_bytes(o) for o in outs])
    for p, run in zip(POISONS[1:], runs[1:]):
        assert len(run) == len(runs[0])
        for k, (a, b) in enumerate(zip(runs[0], run)):
            assert a.shape == b.shape, f"output {k}: {tuple(a.shape)} / {tuple(b.shape)} bytes"
            if not torch.equal(a, b):
                diff = torch.nonzero(a != b).reshape(-1)
                raise AssertionError(f"output {k} depends on what its buffers held before the call: {diff.numel()} bytes "
                                     f"differ between poison 0x{POISONS[0]:02X} and 0x{p:02X}, first at byte "
                                     f"{int(diff[0])} (an element the kernel did not write, or a read of unwritten "
                                     f"scratch)")
    return runs[0], guard_bytes


def assert_same_bytes(got, plain, what="output"):
    """`got` (host byte tensors from same_under_all_poisons) against tensors of a plain, unguarded call."""
    plain = [raw_bytes(t) for t in plain if t is not None]
    assert len(got) == len(plain), f"{what}: {len(got)} guarded outputs, {len(plain)} plain"
    for k, (a, b) in enumerate(zip(got, plain)):
        assert a.shape == b.shape and torch.equal(a, b), \
            f"{what} {k}: {int((a != b).sum()) if a.shape == b.shape else 'all'} bytes differ from the plain call's"


class Plain:
    """The arena's interface on ordinary allocations: the plain, unguarded call the guarded outputs are compared with."""

    def __init__(self, device="cpu"):
        self.device = torch.device(device)

    def carve(self, shape, dtype, role, name=None, guard=None):
        return torch.empty(tuple(shape), dtype=dtype, device=self.device)

    def put(self, src, role="in", name=None):
        return src.to(self.device, copy=True).contiguous()

    def intercept(self, module):
        return contextlib.nullcontext(self)


def guarded_and_plain(arena, fn):
    """same_under_all_poisons, then bit-equality with `fn` on plain allocations -> guard bytes checked per run."""
    got, guard_bytes = same_under_all_poisons(arena, fn)
    outs = fn(Plain(arena.device))
    if arena.device.type == "cuda":
        torch.cuda.synchronize(arena.device)
    assert_same_bytes(got, (outs,) if isinstance(outs, torch.Tensor) else outs)
    return guard_bytes
