"""GPU tier: the attention-matrix backward as row groups on many workgroups plus a c x c tail (rcot_attn_rows_bwd) against its fp64
double (TorchDouble.attn_core_bwd, tests/host_double.py), against the one-launch form (rcot_attn_core_bwd) and, through the block,
against the route that takes the one-launch form at every head width.  dM is handed over dense and as S = 1, 3, 8 and 11 split-K slabs with a leading dimension above C; every
output starts as NaN, the workspace is poisoned, every tensor lies between guard bands.
"""
import ctypes

import pytest
import torch

from conftest import relerr, seeded_tensor
from guarded import GuardSet, all_finite, poison_workspaces
from host_double import TorchDouble

pytestmark = pytest.mark.gpu
DBL = TorchDouble(torch.float64)
EINVAL = -1

# (B, heads, c, group_tiles): the shapes of test_attn_core_bwd under the launcher's rule (0), then one per branch of that rule:
# 15 tiles in groups of 4 (the last one is short), groups of a single tile, and the most tiles for the fewest images
SHAPES = [(2, 1, 48, 0), (2, 2, 48, 0), (8, 8, 48, 0), (2, 1, 96, 0), (1, 4, 96, 0), (3, 2, 96, 0), (2, 4, 24, 0), (8, 4, 48, 0),
          (1, 5, 48, 0), (2, 1, 48, 1), (1, 8, 48, 0)]
FORMS = [0, 1, 3, 8, 11]          # 0: dense; S slabs otherwise


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


def T(seed, *shape, scale=1.0):
    return seeded_tensor(seed, shape, scale=scale)


_cases = {}


def _case(B, heads, c, S):
    """inputs on the host and the double's seven outputs, made once per (shape, S) and left unchanged"""
    key = (B, heads, c, S)
    if key not in _cases:
        C = heads * c
        dM = T(5, B, C, C)
        if S:        # S addends whose (fp64) sum is what the double sees; the kernel adds them in fp32, in slab order
            w = torch.softmax(T(8, S, 1, 1, 1), 0)
            parts = [dM * w[s] for s in range(S - 1)]
            parts.append(dM - sum(parts) if parts else dM.clone())
            slabs = torch.stack(parts, 1)                                        # [B, S, C, C]
            dM = slabs.double().sum(1)
        else:
            slabs = None
        ins = [dM, T(4, C, C, scale=0.1), torch.softmax(T(1, B, heads, c, c, scale=2.0), -1), T(7, B, heads, c, c, scale=0.3),
               T(2, B, 2 * C).abs() * 50 + 1.0, 1 + 0.2 * T(3, heads)]
        outs = [torch.zeros(s, dtype=torch.float64) for s in _out_shapes(B, heads, c)]
        assert DBL.attn_core_bwd(*[t.double() for t in ins], *outs)
        _cases[key] = (ins, slabs, outs)
    return _cases[key]


def _out_shapes(B, heads, c):
    C = heads * c
    return (B, C, C), (B, C, C), (B, heads), (B, heads, c, c), (B, heads, c, c), (B, C), (B, C)


def _rows(be, dM, S, ld, ins, outs, B, heads, c, gt, ws_bytes):
    return be.L.rcot_attn_rows_bwd(dM.data_ptr(), S, ld, *[t.data_ptr() for t in ins], *[t.data_ptr() for t in outs], B, heads, c, gt,
                                   be.ws.data_ptr(), ws_bytes, be._st())


@pytest.mark.parametrize("S", FORMS)
@pytest.mark.parametrize("B,heads,c,gt", SHAPES)
def test_attn_rows_bwd(hip, B, heads, c, gt, S):
    be, C = hip, heads * c
    ins, slabs, ref = _case(B, heads, c, S)
    gs = GuardSet("cuda")
    poison_workspaces(be)
    dev = [gs.tensor(t.float(), f"in[{i}]") for i, t in enumerate(ins)]
    if S:
        ld = C + 4
        dM = gs.full((B, S, C, ld), float("nan"), name="dM slabs")              # the padding columns stay NaN: never read
        dM[..., :C] = slabs.cuda()
    else:
        ld, dM = C, dev[0]
    need = be.L.rcot_attn_rows_ws_bytes(B, heads, c, gt)
    tiles = C // 16
    tpg = min(gt, 4, tiles) if gt else -(-tiles // -(-tiles // 4))
    assert need == B * heads * -(-tiles // tpg) * c * c * 4 and need <= be.ws_bytes
    runs = []
    for _ in range(2):
        outs = [gs.full(s, float("nan")) for s in _out_shapes(B, heads, c)]
        assert _rows(be, dM, S, ld, dev[1:], outs, B, heads, c, gt, need) == 0
        torch.cuda.synchronize()
        runs.append(outs)
    buf = ctypes.create_string_buffer(192)
    be.L.rcot_last_kernel(buf, 192)
    assert buf.value.decode() == f"attn_rows_tail_kernel<{-(-c // 16)}>", buf.value
    for i, (a, b, r) in enumerate(zip(*runs, ref)):
        assert all_finite(a), i
        e = relerr(a, r)
        print(f"output {i}: {e:.2e} of the double")
        assert e < 5e-5, (i, e)
        assert torch.equal(a, b), i                                              # the same bits from run to run
    # the one-launch form on the same inputs (it takes the dense dM)
    old = [gs.full(s, float("nan")) for s in _out_shapes(B, heads, c)]
    from rcot_amd import lib
    lib.check(be.L.rcot_attn_core_bwd(dev[0].data_ptr(), 0, C, *[t.data_ptr() for t in dev[1:]], *[t.data_ptr() for t in old], B, heads, c,
                                      be._st()), "rcot_attn_core_bwd")
    torch.cuda.synchronize()
    for i, (a, o) in enumerate(zip(runs[0], old)):
        e = relerr(a, o)
        print(f"output {i}: {e:.2e} of the one-launch form")
        assert e < 1e-5, (i, e)
    # a workspace one byte short: refused, nothing written
    outs = [gs.full(s, float("nan")) for s in _out_shapes(B, heads, c)]
    assert _rows(be, dM, S, ld, dev[1:], outs, B, heads, c, gt, need - 1) == EINVAL
    torch.cuda.synchronize()
    for t in outs:
        assert bool(torch.isnan(t).all())
    gs.check()


def test_attn_rows_bwd_refuses_what_the_one_launch_form_refuses(hip):
    """(nothing is launched by any of these)"""
    be = hip
    z = torch.zeros(64 * 64, device="cuda")
    p = [z.data_ptr()] * 13
    for heads, c in ((2, 32), (1, 24)):                                           # a head width without a kernel; C no multiple of 16
        assert be.L.rcot_attn_core_bwd(p[0], 0, heads * c, *p[1:], 1, heads, c, be._st()) == -3
        assert be.L.rcot_attn_rows_bwd(p[0], 0, heads * c, *p[1:], 1, heads, c, 0, be.ws.data_ptr(), be.ws_bytes, be._st()) == -3
    assert be.L.rcot_attn_rows_bwd(p[0], 0, 48, *p[1:], 1, 1, 48, 0, 0, be.ws_bytes, be._st()) == EINVAL                 # no workspace
    assert be.L.rcot_attn_rows_ws_bytes(1, 2, 32, 0) == EINVAL


@pytest.mark.parametrize("C,heads", [(96, 1), (96, 2)])
def test_block_backward_row_group_route_vs_parent_route(hip, C, heads):
    """TransformerBlockOp.backward at B = 2, 16x16 with the row-group form forced through the wrapper ("on") against the one-launch
    form forced the same way ("off", c = 48 and c = 96 alike): dx and every parameter gradient, to the bars of
    test_transformer_block_vs_reference_fixture.  The profile of each run names the kernel of its route and not the other's."""
    from rcot_amd import params as P
    from rcot_amd.net_restormer import ParamStore, TransformerBlockOp
    be = hip
    shapes = P.block_param_shapes("blk", C, heads)
    x, gy = seeded_tensor(21, (2, C, 16, 16)).cuda(), seeded_tensor(22, (2, C, 16, 16)).cuda()
    res = {}
    try:
        for route in ("off", "on"):
            be.attn_rows = route
            st = ParamStore(be, shapes, [n for n, _ in shapes], [])
            st.load({k: torch.from_numpy(v) for k, v in P.seeded_params(shapes, 5, "T").items()})
            blk = TransformerBlockOp(be, st, "blk", C, heads)
            blk.repack()
            buf = ctypes.create_string_buffer(1 << 16)
            be.L.rcot_profile_begin()
            _, ctx = blk.forward(x, True)
            dx = blk.backward(ctx, gy)
            be.side_join()
            torch.cuda.synchronize()
            assert be.L.rcot_profile_end(buf, 1 << 16) > 10
            ran = buf.value.decode(errors="replace")
            assert ("attn_rows_tail_kernel" in ran) == (route == "on")
            assert ("attn_bwd_core_kernel" in ran) == (route == "off")
            res[route] = (dx, {n: st.g[n].clone() for n, _ in shapes})
    finally:
        del be.attn_rows
    assert relerr(res["on"][0], res["off"][0]) < 1e-4
    for n, _ in shapes:
        e = relerr(res["on"][1][n], res["off"][1][n])
        assert e < 5e-4, (n, e)
