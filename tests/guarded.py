"""Guard-banded, poisoned buffers for the kernel tests.

A tensor from a ``GuardSet`` is a dense view inside one larger uint8 allocation with a band of ``BAND`` bytes before it and after it
(the slack up to the next 1024-byte boundary behind the tensor belongs to the rear band, byte for byte).  The bands hold a 4-byte
pattern that is a quiet NaN when read as fp32, with a payload of the tensor's own (``0x7FC00000 + 0x100 k`` for the k-th tensor of
the set), so a stray READ of a band surfaces as NaN in what the test compares, and ``check()`` finds a stray WRITE: it compares
every band byte with its pattern as integers and fails with the tensor's name, the side, the offset of the first changed byte
relative to the tensor's first byte (negative in the front band) and the number of changed bytes.

The band width is a multiple of 1024 bytes: the view keeps the 16-byte / 512-byte alignment of the base allocation, so no alignment
refusal and no vector path changes because of the harness.  16 KiB is a condition, not a measurement: wider than the widest row any
kernel here stores in one sweep (1024 floats of an FFT line, 128-column GEMM tiles), so an overrun by a whole tile row still lands
in a band.

``poison_workspaces(backend)`` fills the backend's torch.empty workspaces with NaN in place (launch plans bake their addresses in);
``GuardSet.adopt(backend)`` does that and also routes ``backend.empty`` / ``backend.zeros`` through the set for the duration.
"""
import contextlib

import torch

BAND = 16 * 1024
QNAN = 0x7FC00000
DTYPES = (torch.float32, torch.int32, torch.uint8, torch.float64)


class GuardError(AssertionError):
    def __init__(self, name, side, offset, count):
        super().__init__(f"guard band of {name!r} damaged: {side} the tensor, first changed byte at offset {offset} relative to "
                         f"the tensor, {count} byte(s) changed")
        self.name, self.side, self.offset, self.count = name, side, offset, count


class _Item:
    __slots__ = ("name", "base", "nbytes", "pattern", "view")


class GuardSet:
    def __init__(self, device, band: int = BAND):
        assert band >= BAND and band % 1024 == 0
        self.device, self.band, self.items = torch.device(device), band, []

    # ------------------------------------------------------------------ allocation
    def empty(self, shape, dtype=torch.float32, name=None):
        """a dense [shape] view of ``dtype`` between two bands; the body holds the band pattern too (NaN as fp32)"""
        assert dtype in DTYPES, dtype
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        numel = 1
        for s in shape:
            numel *= s
        it = _Item()
        it.name = name if name is not None else f"#{len(self.items)}"
        it.nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        it.pattern = QNAN + 0x100 * (len(self.items) + 1)
        assert it.pattern < 0x7FFFFFFF
        body = -(-it.nbytes // 1024) * 1024
        it.base = torch.empty(self.band + body + self.band, dtype=torch.uint8, device=self.device)
        it.base.view(torch.int32).fill_(it.pattern)
        it.view = it.base[self.band:self.band + it.nbytes].view(dtype).view(shape)
        assert it.view.data_ptr() == it.base.data_ptr() + self.band
        self.items.append(it)
        return it.view

    def tensor(self, host, name=None):
        """a guarded copy of ``host`` (any strides; the copy is dense)"""
        v = self.empty(host.shape, host.dtype, name)
        v.copy_(host)
        return v

    def full(self, shape, value, dtype=torch.float32, name=None):
        v = self.empty(shape, dtype, name)
        v.fill_(value)
        return v

    # ------------------------------------------------------------------ the check
    def _bands(self, it):
        """(side, band bytes, expected bytes, offset of the band's first byte relative to the tensor) for both bands"""
        pat = torch.tensor([it.pattern], dtype=torch.int32, device=self.device).view(torch.uint8)
        n_back = it.base.numel() - self.band - it.nbytes
        phase = it.nbytes % 4                                  # the rear band starts inside a pattern word for odd-sized tensors
        exp_back = pat.repeat(n_back // 4 + 2)[phase:phase + n_back]
        return (("before", it.base[:self.band], pat.repeat(self.band // 4), -self.band),
                ("after", it.base[self.band + it.nbytes:], exp_back, it.nbytes))

    def check(self):
        """every band byte against its pattern, as integers; raises GuardError for the first damaged band"""
        if not self.items:
            return
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        bands = [(it, *b) for it in self.items for b in self._bands(it)]
        counts = torch.stack([(got != exp).sum() for _, _, got, exp, _ in bands]).cpu().tolist()   # one transfer for the clean case
        for (it, side, got, exp, off), n in zip(bands, counts):
            if n:
                first = int(torch.nonzero(got != exp)[0, 0])
                raise GuardError(it.name, side, off + first, int(n))

    # ------------------------------------------------------------------ whole paths: the backend allocates from the set
    @contextlib.contextmanager
    def adopt(self, backend):
        """inside: ``backend.empty`` returns a guarded NaN-filled body, ``backend.zeros`` a guarded one cleared by ``backend.fill``
        as now, and the workspaces start as NaN.  On exit the two methods are restored and the set is checked.  (The zero-initialised
        operand buffers of ``_pcm_buffer`` are left alone: their zeros are part of the contract.)"""
        count = [0]

        def empty(*shape):
            if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
                shape = tuple(shape[0])
            count[0] += 1
            return self.empty(shape, torch.float32, f"backend.empty #{count[0]} {tuple(shape)}")

        def zeros(*shape):
            t = empty(*shape)
            if t.numel():
                backend.fill(t, 0.0)
            return t

        poison_workspaces(backend)
        backend.empty, backend.zeros = empty, zeros
        try:
            yield self
        finally:
            del backend.empty, backend.zeros
        self.check()


def poison_workspaces(backend):
    """NaN into ``backend.ws``, ``_ws_side``, both ``_ws_slabs_gen`` and the four ``_ln_scratch`` buffers, in place"""
    bufs = [backend.ws, backend._ws_side, *backend._ws_slabs_gen, *(t for pair in backend._ln_scratch for t in pair)]
    for t in bufs:
        if t is not None:
            t.fill_(float("nan"))


def all_finite(t) -> bool:
    return bool(torch.isfinite(t).all())
