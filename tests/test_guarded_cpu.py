"""The guard-band harness (tests/guarded.py) checked on host memory: a check that cannot fail is worth nothing.  The damage is done
with a torch copy into the base allocation, never by a kernel.  tests/test_guards_gpu.py runs ``selftest`` again on the device.
Also here: the alignment refusals of the entry points that load float4 from a caller's pointer (they return before any launch)."""
import numpy as np
import pytest
import torch

from guarded import BAND, QNAN, GuardError, GuardSet


def selftest(device):
    gs = GuardSet(device)
    img = gs.tensor(torch.arange(37 * 45 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(37, 45, 3), "img")
    x = gs.tensor(torch.linspace(-1, 1, 1000).view(10, 100), "x")
    idx = gs.empty((7,), torch.int32, "idx")
    acc = gs.empty((4,), torch.float64, "acc")
    assert img.shape == (37, 45, 3) and img.dtype == torch.uint8 and img.is_contiguous() and x.is_contiguous()
    assert idx.dtype == torch.int32 and acc.dtype == torch.float64 and acc.shape == (4,)
    its = {it.name: it for it in gs.items}
    for it in gs.items:
        assert it.view.data_ptr() - it.base.data_ptr() == BAND and BAND % 1024 == 0 and BAND >= 16384
        assert it.view.data_ptr() % 16 == it.base.data_ptr() % 16 and it.view.data_ptr() % 512 == it.base.data_ptr() % 512
        assert it.base.numel() - BAND - it.nbytes >= BAND
        word = it.base[:4].view(torch.int32).item()
        assert word == it.pattern and word >= QNAN and bool(torch.isnan(it.base[:4].view(torch.float32)).all())
    assert len({it.pattern for it in gs.items}) == len(gs.items)
    assert bool(torch.isnan(gs.empty((5,), torch.float32, "fresh")).all())          # a fresh body is NaN as well
    gs.check()                                                                      # clean

    # a changed element inside a tensor is not reported
    img[36, 44, 2] = 7
    x[0, 0] = 3.0
    x[9, 99] = float("nan")
    gs.check()

    # one byte just past the 37 x 45 x 3 uint8 image: 4995 bytes, so the byte sits in the slack before the next 1024-byte boundary
    base = its["img"].base
    p = BAND + 37 * 45 * 3
    old = base[p:p + 1].clone()
    base[p:p + 1].copy_(torch.tensor([0x5A], dtype=torch.uint8))
    with pytest.raises(GuardError) as e:
        gs.check()
    assert (e.value.name, e.value.side, e.value.offset, e.value.count) == ("img", "after", 4995, 1)
    assert "img" in str(e.value) and "4995" in str(e.value)
    base[p:p + 1].copy_(old)
    gs.check()

    # one float just before the fp32 tensor
    base = its["x"].base
    old = base[BAND - 4:BAND].clone()
    base[BAND - 4:BAND].view(torch.float32).copy_(torch.tensor([1.0]))               # 00 00 80 3F against 00 xx C0 7F
    with pytest.raises(GuardError) as e:
        gs.check()
    changed = int((base[BAND - 4:BAND].cpu() != old.cpu()).sum())
    assert changed >= 2
    first = -4 + int(torch.nonzero(base[BAND - 4:BAND].cpu() != old.cpu())[0, 0])
    assert (e.value.name, e.value.side, e.value.offset, e.value.count) == ("x", "before", first, changed)
    base[BAND - 4:BAND].copy_(old)
    gs.check()

    # the last byte of a rear band and a value carried over from ANOTHER tensor's band are both seen
    base = its["acc"].base
    old = base[-1:].clone()
    base[-1:].copy_(torch.tensor([0], dtype=torch.uint8))
    with pytest.raises(GuardError) as e:
        gs.check()
    assert (e.value.name, e.value.side, e.value.offset, e.value.count) == ("acc", "after", base.numel() - BAND - 1, 1)
    base[-1:].copy_(old)
    base[:4].copy_(its["idx"].base[:4])
    with pytest.raises(GuardError) as e:
        gs.check()
    assert (e.value.name, e.value.side, e.value.offset) == ("acc", "before", -BAND + 1)   # the payload byte differs
    return True


def test_guardset_on_host_memory():
    assert selftest("cpu")


def test_adopt_patches_the_instance_and_restores_it():
    class Backend:
        def __init__(self):
            self.ws = torch.zeros(64)
            self._ws_side = None
            self._ws_slabs_gen = [torch.zeros(8), torch.zeros(8)]
            self._ln_scratch = [[torch.zeros(4) for _ in range(2)] for _ in range(2)]
            self.filled = []

        def empty(self, *shape):
            return torch.empty(*shape)

        def zeros(self, *shape):
            return torch.zeros(*shape)

        def fill(self, t, v):
            self.filled.append(t.data_ptr())
            t.fill_(v)

    be = Backend()
    addr = be.ws.data_ptr()
    gs = GuardSet("cpu")
    with gs.adopt(be):
        assert be.ws.data_ptr() == addr and bool(torch.isnan(be.ws).all()) and bool(torch.isnan(be._ln_scratch[1][1]).all())
        e, z = be.empty(3, 5), be.zeros(2, 2)
        assert e.shape == (3, 5) and bool(torch.isnan(e).all()) and float(z.abs().sum()) == 0.0 and be.filled == [z.data_ptr()]
        assert len(gs.items) == 2
    assert "empty" not in vars(be) and "zeros" not in vars(be) and be.empty(2).shape == (2,)
    gs2 = GuardSet("cpu")
    with pytest.raises(GuardError):
        with gs2.adopt(be):
            t = be.empty(4)
            gs2.items[0].base[BAND + 16:BAND + 17].copy_(torch.tensor([1], dtype=torch.uint8))
    assert "empty" not in vars(be)


# ------------------------------------------------------------------ alignment refusals (no launch: no device needed)
@pytest.fixture(scope="module")
def addr():
    """a 16-byte aligned address no kernel will touch (every call below returns before its launch)"""
    keep = np.zeros(4096 + 4, np.float32)
    return keep, (keep.ctypes.data + 15) // 16 * 16


def test_row_sumsq_refuses_a_misaligned_operand(addr):
    """include/rcot_hip.h promises RCOT_EINVAL for bad alignment; row_sumsq_kernel loads float4 from x"""
    from rcot_amd import lib
    L = lib.load()
    a = addr[1]
    for off in (4, 8, 12):
        assert L.rcot_row_sumsq(a + off, a + 8192, 1, 1, 4, 4, None) == -1, off
    assert L.rcot_row_sumsq(a, a + 8192, 1, 1, 6, 8, None) == -1                   # N & 3, as before
    assert L.rcot_row_sumsq(a, a + 8192, 1, 1, 4, 6, None) == -1                   # sXb & 3, as before
    assert L.rcot_row_sumsq(None, a + 8192, 1, 1, 4, 4, None) == -1


def test_float4_stencils_and_ln_bwd_refuse_misaligned_operands(addr):
    """the same omission in the other entry points of csrc/pointwise.hip and csrc/stencil.hip that cast a caller's pointer to float4: each vector-accessed
    operand, 4 bytes off, is refused; planes with a side that is no multiple of 4 take scalar kernels and are not asked for it"""
    from rcot_amd import lib
    L = lib.load()
    a = addr[1]
    q = [a + 1024 * i for i in range(12)]
    calls = {
        "rcot_ln_bwd": (lambda p: L.rcot_ln_bwd(p[0], p[1], p[2], p[3], q[4], p[5], p[6], None, None, 1, 4, 4, q[7], 4096, None),
                        (0, 1, 2, 3, 5, 6)),
        "rcot_dwconv3x3": (lambda p: L.rcot_dwconv3x3(p[0], q[1], p[2], 1, 1, 4, 4, 0, None), (0, 2)),
        "rcot_gdfn_gate_fwd": (lambda p: L.rcot_gdfn_gate_fwd(p[0], q[1], p[2], 1, 1, 4, 4, None), (0, 2)),
        "rcot_gdfn_gate_bwd": (lambda p: L.rcot_gdfn_gate_bwd(p[0], q[1], p[2], p[3], None, 1, 1, 4, 4, None), (0, 2, 3)),
        "rcot_dwconv3x3_wgrad": (lambda p: L.rcot_dwconv3x3_wgrad(p[0], p[1], q[2], 1, 1, 4, 4, None), (0, 1)),
        "rcot_gdfn_bwd": (lambda p: L.rcot_gdfn_bwd(p[0], q[1], p[2], p[3], q[4], p[5], 1, 1, 4, 4, None), (0, 2, 3, 5)),
        "rcot_dwconv3x3_bwd": (lambda p: L.rcot_dwconv3x3_bwd(p[0], p[1], q[2], p[3], q[4], 1, 1, 4, 4, None), (0, 1, 3)),
    }
    for name, (call, vec) in calls.items():
        for i in vec:
            p = list(q)
            p[i] += 4
            assert call(p) == -1, (name, i)
