"""GPU tier: the strip kernels of csrc/stencil.hip at the smallest planes at which a row requested ahead of its use can go wrong.

The strip kernels request rows before they use them, from CLAMPED row indices, and zero what lies outside the plane when it lands;
`dwconv_bwd_kernel<*, 4, true>` asks for all six rows of its strip before its first arithmetic.  A clamp that is off by one reads a row
of the neighbouring plane (or the guard band: NaN) into a halo, a mask that is off by one keeps a row that should be zero.  So: planes
of one strip (every halo row clamped), of two and three strips, one column group (no neighbour lanes) and several (lane halos), one
wavefront and one workgroup per plane, more than one plane and batch entry everywhere but in the first case — against the fp64
double at the tolerance of test_gdfn_bwd_one_pass (fp32 rounding only, 2e-5 of max|ref|), through `both()` of test_kernels_gpu.py:
every operand and result in a guard-banded buffer (NaN bands, checked bit for bit), workspaces poisoned.
"""
import pytest

from test_kernels_gpu import T, _last_kernel, _strip_ladder, both, hip  # noqa: F401  (hip: the module-scoped backend fixture)

import torch

pytestmark = pytest.mark.gpu

# (B, planes per batch entry, H, W): one strip and one column group (every halo row clamped, no neighbour lane); two strips, no
# neighbour lanes; one strip with lane halos; three strips (12 threads per plane: no lane grouping fits, the unfused routes);
# one wavefront per plane; one workgroup per plane
SMALL = [(1, 1, 4, 4), (2, 3, 8, 4), (1, 2, 4, 16), (2, 5, 12, 16), (1, 3, 16, 64), (1, 2, 64, 64)]
# 8-row strips (the smallest shapes that reach them: test_gdfn_bwd_one_pass_tall_strips): ragged sub-wave groups, one wavefront
TALL = [(2, 12500, 12, 16), (1, 1563, 64, 64)]


def gate_operands(B, hid, H, W):
    return [T(1, B, 2 * hid, H, W), T(2, 2 * hid, 9, scale=0.5), T(3, B, hid, H, W), torch.zeros(B, 2 * hid, H, W), T(4, 2 * hid, 9)]


@pytest.mark.parametrize("B,hid,H,W", SMALL + TALL)
def test_gdfn_bwd_rows_requested_ahead(hip, B, hid, H, W):
    G, RS, _ = _strip_ladder(B * hid, H, W, 200000)
    assert RS == (8 if (B, hid, H, W) in TALL else 4)

    def fn(be, p, w, dg, dp, dw):
        be.gdfn_bwd(p, w, dg, dp, dw)
        if be is hip and G:
            assert _last_kernel(hip) == f"gdfn_bwd_kernel<{G}, {RS}>"
    both(hip, fn, gate_operands(B, hid, H, W), [3, 4])


@pytest.mark.parametrize("B,hid,H,W", SMALL)
def test_gdfn_gate_bwd_with_weight_gradient_small_planes(hip, B, hid, H, W):
    assert _strip_ladder(B * hid, H, W, 400000)[1] == 4

    def fn(be, p, w, dg, dd, dw):
        be.gdfn_gate_bwd(p, w, dg, dd, dw=dw)
    both(hip, fn, gate_operands(B, hid, H, W), [3, 4])


@pytest.mark.parametrize("B,C,H,W", SMALL)
def test_dwconv_bwd_whole_strip_requested_ahead(hip, B, C, H, W):
    assert _strip_ladder(B * C, H, W, 400000)[1] == 4

    def fn(be, dy, x, w, dx, dw):
        be.dwconv3x3_bwd(dy, x, w, dx, dw)
    both(hip, fn, [T(1, B, C, H, W), T(2, B, C, H, W), T(3, C, 9), torch.zeros(B, C, H, W), T(4, C, 9)], [3, 4])
