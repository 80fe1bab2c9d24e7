"""TEST INFRASTRUCTURE ONLY (host side of tests/test_gpu_bounds.py, in the style of tests/stale_memory.py): allocators and input
placement that put all-ones GUARD BANDS around every buffer a wrapper hands to the library.

include/rohm_hip.h promises that a call touches only the operands it is given, and of a workspace only as many bytes as its
`*_bytes` function says.  With tightly sized tensors a store one row past a buffer lands in the caching allocator's rounding or in a
neighbouring tensor, and a load there returns finite leftovers: nothing notices.  Here

  * `guard()` replaces torch.empty, torch.empty_like, Tensor.new_empty, torch.zeros and Tensor.new_zeros: what they return is a view into
    the middle of a larger flat uint8 buffer -- BAND bytes of 0xFF (fp32 / fp64 NaN, integer -1) in front, the zero-filled interior,
    then 0xFF padding up to the next multiple of 512 bytes and BAND more bytes of 0xFF.  The view has the dtype and shape that were
    asked for and a 512-byte-aligned address -- or, with `guard(offset=True)`, an address one element of its own dtype past such a
    boundary, the least alignment the headers promise to accept.  A store outside the interior changes a band byte (`violations()`);
    a load there is NaN and shows in the result.
  * `place(t, placement)` puts an INPUT tensor into a flat device buffer of 0xFF bytes with BAND bytes on either side (`Canvas`), so a
    read past an input is NaN as well and a write to an input is seen (`untouched()`).

BAND = 1 MiB: more than one 144-row tile of the widest row the library stages, 144 x 1536 floats = 884,736 bytes.  A stray access
FURTHER OUT than BAND bytes from the buffer is not seen by either tool.  A stray LOAD shows only through the result: 0 x NaN is still
NaN, so a value that is multiplied in shows; one that is only compared (fmaxf, a mask) may not.  And a stray STORE of a value that
was itself loaded from a band is not seen where both bands hold the same NaN (arithmetic hands a quiet NaN on with its bits):
`Canvas(band=...)` gives the inputs another NaN where a test has to see such a store."""
import contextlib

import torch

import stale_memory as SM

BAND = 1 << 20
ALIGN = 512
_REAL = {'empty': torch.empty, 'empty_like': torch.empty_like, 'new_empty': torch.Tensor.new_empty, 'zeros': torch.zeros,
         'new_zeros': torch.Tensor.new_zeros, 'full': torch.full}
_REAL_FILL = SM.fill_bytes


def _flat(nbytes, device):
    """A flat uint8 buffer of 0xFF bytes and the offset `front` >= BAND inside it at which a 512-byte-aligned interior of `nbytes`
    bytes starts; behind the interior lie the pad bytes up to a multiple of 512 and BAND more bytes."""
    padded = (nbytes + ALIGN - 1) // ALIGN * ALIGN
    flat = _REAL['full']((BAND + ALIGN + padded + BAND,), 0xFF, dtype=torch.uint8, device=device)
    front = BAND + (-(flat.data_ptr() + BAND)) % ALIGN
    return flat, front


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _size_of(args, kwargs):
    """The size of torch.empty(*size) / torch.empty(size) / torch.empty(size=size) as a tuple of ints, or None."""
    if 'size' in kwargs:
        size = kwargs['size']
    elif len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        size = args[0]
    else:
        size = args
    try:
        return tuple(int(s) for s in size)
    except (TypeError, ValueError):
        return None


class _Record:
    """One served allocation: the flat buffer (kept alive), where its interior lies, and what was asked for."""

    def __init__(self, kind, flat, front, nbytes, shape, dtype):
        self.kind, self.flat, self.front, self.nbytes, self.shape, self.dtype = kind, flat, front, nbytes, tuple(shape), dtype

    def describe(self):
        return f'{self.kind}{list(self.shape)} {str(self.dtype).replace("torch.", "")} ({self.nbytes} bytes)'

    def bands(self):
        return self.flat[:self.front], self.flat[self.front + self.nbytes:]


class Guard:
    """The state of one `guard()`: `records` (every served allocation, in order), `served`, `unguarded` (the number of allocations passed
    through to torch unchanged) and `passed_through` (what they were)."""

    def __init__(self, device_types, offset=False):
        self.device_types, self.offset = tuple(device_types), bool(offset)
        self.records = []
        self.passed_through = []
        self._by_storage = {}

    @property
    def served(self):
        return len(self.records)

    @property
    def unguarded(self):
        return len(self.passed_through)

    def log(self):
        """[(kind, shape, dtype, nbytes)] of the served allocations, in order."""
        return [(r.kind, r.shape, r.dtype, r.nbytes) for r in self.records]

    # ---- serving
    def wants(self, device):
        return torch.device(device).type in self.device_types

    def serve(self, kind, shape, dtype, device, strides=None, requires_grad=False):
        nbytes = _numel(shape) * _itemsize(dtype)
        lead = _itemsize(dtype) if self.offset else 0
        flat, front = _flat(lead + nbytes, device)
        front += lead
        inner = flat[front:front + nbytes]
        inner.zero_()
        typed = inner.view(dtype)
        out = typed.view(shape) if strides is None else typed.as_strided(shape, strides)
        assert out.data_ptr() % ALIGN == lead or nbytes == 0
        rec = _Record(kind, flat, front, nbytes, shape, dtype)
        self.records.append(rec)
        self._by_storage[flat.untyped_storage().data_ptr()] = rec
        if requires_grad:
            out.requires_grad_(True)
        return out

    def refuse(self, kind, why, real, args, kwargs):
        out = real(*args, **kwargs)
        if torch.is_tensor(out) and self.wants(out.device):
            self.passed_through.append(f'{kind}: {why}')
        return out

    def fill_interior(self, t, word):
        """stale_memory.fill_bytes for a tensor this guard served: the pattern goes into the interior only (a case that poisons its own
        set-up, e.g. `with SM.poison(SM.ZEROS)`, must not wipe the bands)."""
        rec = self._by_storage.get(t.untyped_storage().data_ptr()) if t.untyped_storage().nbytes() else None
        if rec is None:
            return _REAL_FILL(t, word)
        if rec.nbytes:
            inner = rec.flat[rec.front:rec.front + rec.nbytes]
            if len(set(word)) == 1:
                inner.fill_(word[0])
            else:
                inner.copy_(torch.tensor(list(word), dtype=torch.uint8, device=inner.device).repeat((rec.nbytes + 3) // 4)[:rec.nbytes])
        return t

    # ---- checking
    def violations(self):
        """After a device synchronisation: [(index, description, offset)] of every served allocation whose bands are no longer all
        0xFF; `offset` is that of the first changed byte relative to the interior's first byte (negative: in front of it; >= the
        allocation's bytes: behind it).  The bands are tested against 0xFF; no copies are kept."""
        if torch.cuda.is_available() and 'cuda' in self.device_types:
            torch.cuda.synchronize()
        if not self.records:
            return []
        flags = {}
        for i, r in enumerate(self.records):
            a, b = r.bands()
            flags.setdefault(r.flat.device, []).append((i, (a != 0xFF).any() | (b != 0xFF).any()))
        bad = []
        for items in flags.values():
            hit = torch.stack([f for _, f in items]).cpu().tolist()
            bad += [i for (i, _), h in zip(items, hit) if h]
        out = []
        for i in sorted(bad):
            r = self.records[i]
            a, b = r.bands()
            ia = (a != 0xFF).nonzero()
            off = int(ia[0]) - r.front if ia.numel() else r.nbytes + int((b != 0xFF).nonzero()[0])
            out.append((i, r.describe(), off))
        return out


def _itemsize(dtype):
    return _REAL['empty']((), dtype=dtype).element_size()


def _default_device():
    return torch.get_default_device() if hasattr(torch, 'get_default_device') else torch.device('cpu')


def _plain_kwargs(kwargs, allow_format):
    """None if the keyword arguments describe an allocation `Guard.serve` can make, else the reason it cannot."""
    if kwargs.get('out') is not None:
        return 'out='
    if kwargs.get('pin_memory'):
        return 'pinned memory'
    if kwargs.get('layout') not in (None, torch.strided):
        return 'a layout other than strided'
    if kwargs.get('names') is not None:
        return 'named dimensions'
    fmt = kwargs.get('memory_format')
    if fmt is not None and fmt not in allow_format:
        return f'memory_format {fmt}'
    return None


def install(monkeypatch, g):
    """Replace the five allocators until `monkeypatch` is undone; `g` (a Guard) serves tensors on its device types."""

    def creator(kind, real):
        def create(*a, **k):
            why = _plain_kwargs(k, (torch.contiguous_format,))
            device = k.get('device')
            device = _default_device() if device is None else torch.device(device)
            if not g.wants(device):
                return real(*a, **k)
            size = _size_of(a, k)
            if why is None and size is None:
                why = 'a size that is not a list of integers'
            if why is not None:
                return g.refuse(kind, why, real, a, k)
            dtype = k.get('dtype') or torch.get_default_dtype()
            return g.serve(kind, size, dtype, device, requires_grad=bool(k.get('requires_grad')))
        return create

    def method(kind, real):
        def create(self, *a, **k):
            why = _plain_kwargs(k, ())
            device = torch.device(k['device']) if k.get('device') is not None else self.device
            if not g.wants(device):
                return real(self, *a, **k)
            size = _size_of(a, k)
            if why is None and size is None:
                why = 'a size that is not a list of integers'
            if why is not None:
                return g.refuse(kind, why, lambda *aa, **kk: real(self, *aa, **kk), a, k)
            return g.serve(kind, size, k.get('dtype') or self.dtype, device, requires_grad=bool(k.get('requires_grad')))
        return create

    def empty_like(t, *a, **k):
        real = _REAL['empty_like']
        device = torch.device(k['device']) if k.get('device') is not None else t.device
        if not g.wants(device):
            return real(t, *a, **k)
        why = _plain_kwargs(k, (torch.contiguous_format, torch.preserve_format))
        if why is None and a:
            why = 'positional options'
        strides = None
        if why is None and k.get('memory_format') is not torch.contiguous_format and not t.is_contiguous():
            # preserve_format keeps the strides of an input that is dense and does not overlap itself
            span = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride())) if t.numel() else 0
            if span == t.numel() and all(st > 0 for st in t.stride()):
                strides = t.stride()
            else:
                why = 'preserve_format of an input that is not dense'
        if why is not None:
            return g.refuse('empty_like', why, lambda *aa, **kk: real(t, *aa, **kk), a, k)
        return g.serve('empty_like', tuple(t.shape), k.get('dtype') or t.dtype, device, strides=strides,
                       requires_grad=bool(k.get('requires_grad')))

    monkeypatch.setattr(torch, 'empty', creator('empty', _REAL['empty']))
    monkeypatch.setattr(torch, 'zeros', creator('zeros', _REAL['zeros']))
    monkeypatch.setattr(torch, 'empty_like', empty_like)
    monkeypatch.setattr(torch.Tensor, 'new_empty', method('new_empty', _REAL['new_empty']))
    monkeypatch.setattr(torch.Tensor, 'new_zeros', method('new_zeros', _REAL['new_zeros']))
    monkeypatch.setattr(SM, 'fill_bytes', g.fill_interior)


@contextlib.contextmanager
def guard(device_types=('cuda',), offset=False):
    """The guarded allocators as a context manager (its own MonkeyPatch, undone on exit) -> the `Guard`.  Every flat buffer stays alive
    until exit (and as long as the Guard is), so no band is recycled while the case runs.  `offset`: every allocation starts one
    element of its own dtype past a 512-byte boundary instead of on it."""
    import pytest
    g = Guard(device_types, offset)
    with pytest.MonkeyPatch.context() as m:
        install(m, g)
        yield g


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
class Canvas:
    """A flat buffer of 0xFF bytes holding one input tensor (`view`) with BAND bytes on either side, and a copy of the whole buffer
    taken at placement.  placement 'aligned': the first element lies on a 512-byte boundary.  placement 'slice' ([B, 294, 1, T] float32
    only): the canvas holds B + 1 clips, the first of them all 0xFF on a 512-byte boundary, and the operand is clips 1 .. B -- what a
    caller who passes `batch[1:]` hands in: 8 bytes past a 16-byte boundary for T = 143 and T = 63.  placement 'offset': the first
    element lies one element past a 512-byte boundary (4 bytes for float32, 8 for float64), the 0xFF element in front of it is band."""

    def __init__(self, t, placement='aligned', device=None, label=None, band=SM.PATTERNS['ones']):
        """`band`: the 4-byte word the bytes around the operand repeat (little-endian).  The default is all-ones; a test that must
        SEE a store of what was loaded from a band into a `guard()` band uses another NaN, e.g. 0x7FC00001: the hardware hands a
        quiet NaN through its arithmetic with its bits unchanged, so all-ones stored onto all-ones changes nothing."""
        device = t.device if device is None else torch.device(device)
        t = t.detach()
        if not t.is_contiguous():
            raise ValueError('Canvas takes contiguous tensors')
        nbytes = t.numel() * t.element_size()
        lead = 0
        if placement == 'slice':
            if t.dim() != 4 or t.shape[1] != 294 or t.shape[2] != 1 or t.dtype != torch.float32:
                raise ValueError(f"placement 'slice' is for [B, 294, 1, T] float32 operands, got {t.dtype} {tuple(t.shape)}")
            lead = 294 * int(t.shape[3]) * 4
        elif placement == 'offset':
            lead = t.element_size()
        elif placement != 'aligned':
            raise ValueError(f'unknown placement {placement!r}')
        self.flat, front = _flat(lead + nbytes, device)
        if bytes(band) != SM.PATTERNS['ones']:
            self.flat.view(torch.int32).fill_(int.from_bytes(bytes(band), 'little', signed=True))
        self.offset, self.nbytes, self.placement, self.label = front + lead, nbytes, placement, label
        inner = self.flat[self.offset:self.offset + nbytes]
        if nbytes:
            inner.copy_(t.reshape(-1).view(torch.uint8))
        self.view = inner.view(t.dtype).view(t.shape)
        self.shape, self.dtype = tuple(t.shape), t.dtype
        self.copy = self.flat.clone()

    def untouched(self):
        """Whether every byte of the buffer, operand and bands, still equals the copy taken at placement."""
        return bool(torch.equal(self.flat, self.copy))

    def bands_untouched(self):
        """Whether the bytes around the operand still equal the copy (for an operand the call updates in place)."""
        a, b = self.offset, self.offset + self.nbytes
        return bool(torch.equal(self.flat[:a], self.copy[:a])) and bool(torch.equal(self.flat[b:], self.copy[b:]))

    def first_change(self):
        """None, or the offset of the first changed byte relative to the operand's first byte."""
        d = (self.flat != self.copy).nonzero()
        return int(d[0]) - self.offset if d.numel() else None

    def describe(self):
        return f'{self.label or "canvas"}{list(self.shape)} {str(self.dtype).replace("torch.", "")} ({self.placement})'


def place(t, placement='aligned', device=None, into=None, label=None, band=SM.PATTERNS['ones']):
    """`t` (any dtype, contiguous) on `device` (default: where it is) inside a `Canvas` -> the operand view.  The Canvas is appended to the
    list `into`."""
    c = Canvas(t, placement, device, label, band)
    if into is not None:
        into.append(c)
    return c.view
