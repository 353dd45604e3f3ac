"""Guard bands and poisoned buffers for tests/test_gpu_memory_discipline.py: what the kernels do to memory they should
neither read nor write.

``guarded_empty(pattern)`` replaces ``torch.empty`` while it is active.  Every CUDA tensor asked of it is an interior,
contiguous view of a larger uint8 allocation ``[front guard | payload | back guard]``: both guards at least 64 KiB (more
than one 4096-point complex float64 tile row, the largest unit a kernel here strides by), the payload 256-byte aligned,
all of it filled with one byte.  A slot a kernel reads without having written it then holds the pattern instead of the
allocator's leftovers, and a store outside the tensor lands in a guard, which ``violations()`` reports after the block.
``guarded(t, pattern)`` embeds a tensor of the caller's (x, w, b, dY) the same way, optionally at an address that is only
element-aligned.  ``same_bits`` compares two tensors through an integer view.

The byte patterns, each meaningful for every dtype the library takes:
    0x00  zeros, the baseline;
    0xFF  a NaN in float16, bfloat16, float32 and float64;
    0x7F  a huge finite value in float32 (3.39e38), float64 (1.4e306) and bfloat16 (3.39e38); a NaN in float16."""
import torch

GUARD_BYTES = 64 * 1024
ALIGN = 256
PATTERNS = (0x00, 0xFF, 0x7F)

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_REAL_EMPTY = torch.empty


class _Block:
    """One allocation [front guard | payload | back guard] of uint8, filled with ``pattern``."""

    def __init__(self, alloc, shape, dtype, device, pattern, offset_elems=0):
        self.shape, self.dtype, self.pattern = tuple(int(s) for s in shape), dtype, pattern
        item = torch.zeros(0, dtype=dtype).element_size()
        n = 1
        for s in self.shape:
            n *= s
        self.nbytes = n * item
        total = 2 * GUARD_BYTES + self.nbytes + ALIGN + offset_elems * item
        self.buf = alloc(total, dtype=torch.uint8, device=device)
        self.buf.fill_(pattern)
        self.start = GUARD_BYTES + (-(self.buf.data_ptr() + GUARD_BYTES)) % ALIGN + offset_elems * item
        payload = self.buf[self.start:self.start + self.nbytes]
        self.view = payload.view(dtype).view(self.shape)

    def violations(self):
        """(shape, dtype, "front" | "back", offset) per damaged guard: the byte offset of its first (lowest) changed byte
        from the first byte of the payload -- negative in the front guard, at least the payload's size in the back one."""
        found = []
        end = self.start + self.nbytes
        for which, lo, hi in (("front", 0, self.start), ("back", end, self.buf.numel())):
            bad = (self.buf[lo:hi] != self.pattern).nonzero()
            if bad.numel():
                found.append((self.shape, self.dtype, which, lo + int(bad[0]) - self.start))
        return found


class guarded_empty:
    """Context manager: ``torch.empty`` serves CUDA requests (and CPU ones with ``cpu=True``, for the host check of this
    helper) from guarded, pattern-filled blocks.  Other factories and other devices pass through.  After the block
    (and a ``torch.cuda.synchronize()``) ``violations()`` lists the guards that no longer hold the pattern."""

    def __init__(self, pattern, cpu=False):
        assert 0 <= pattern <= 0xFF
        self.pattern, self.cpu = pattern, cpu
        self.served = []          # (shape, dtype) of every allocation handed out
        self._blocks = []
        self._violations = None

    def _serves(self, device):
        if device is None:
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
        kind = torch.device(device).type if not isinstance(device, int) else "cuda"
        return kind == "cuda" or (kind == "cpu" and self.cpu)

    def _empty(self, *size, **kw):
        device = kw.get("device")
        plain = set(kw) <= {"dtype", "device", "requires_grad", "size"} and kw.get("layout") is None
        if not plain or not self._serves(device):
            return self._real(*size, **kw)
        if "size" in kw:
            size = (kw["size"],)
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        dtype = kw.get("dtype") or torch.get_default_dtype()
        block = _Block(self._real, shape, dtype, device, self.pattern)
        self._blocks.append(block)
        self.served.append((block.shape, dtype))
        out = block.view
        return out.requires_grad_() if kw.get("requires_grad") else out

    def __enter__(self):
        self._real = torch.empty
        torch.empty = self._empty
        return self

    def __exit__(self, *exc):
        torch.empty = self._real
        if torch.cuda.is_available() and any(b.buf.is_cuda for b in self._blocks):
            torch.cuda.synchronize()
        self._violations = [v for b in self._blocks for v in b.violations()]
        self._blocks = []         # (the views handed out keep their blocks alive)
        return False

    def violations(self):
        assert self._violations is not None, "violations() is read after the block"
        return list(self._violations)


def guarded(t, pattern, offset=0):
    """``t`` copied into a guarded block of its own -> (the interior view, checker).  ``offset``: elements by which the
    payload starts past its 256-byte boundary (1: an address that is only element-aligned).  ``checker()`` synchronises
    and returns the block's guard violations, plus a ("payload") entry if the copy no longer has ``t``'s bits: kernels do
    not write their inputs."""
    src = t.detach().contiguous()
    block = _Block(_REAL_EMPTY, src.shape, src.dtype, src.device, pattern, offset)
    block.view.copy_(src)
    assert block.view.is_contiguous() and block.view.data_ptr() % ALIGN == (offset * src.element_size()) % ALIGN

    def check():
        if src.is_cuda:
            torch.cuda.synchronize()
        found = block.violations()
        a, b = _as_int(block.view), _as_int(src)
        if not torch.equal(a, b):
            found.append((block.shape, block.dtype, "payload", int((a != b).flatten().nonzero()[0]) * src.element_size()))
        return found
    return block.view, check


def _as_int(t):
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t.resolve_conj().resolve_neg())
    return t.contiguous().view(_INT_VIEW[t.element_size()])


def same_bits(a, b, what):
    """Bit equality through an integer view of the dtype (-0.0 is not 0.0, NaN payloads count); the failure names how many
    elements differ and the first."""
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}"
    ia, ib = _as_int(a), _as_int(b)
    if torch.equal(ia, ib):
        return
    ne = ia != ib
    first = int(ne.flatten().nonzero()[0])
    index, rest = [], first
    for dim in reversed(ne.shape):
        index.insert(0, rest % dim)
        rest //= dim
    raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ in their bits, the first at "
                         f"{tuple(index)} ({a.dtype}: {ia.flatten()[first].item():#x} vs {ib.flatten()[first].item():#x})")
