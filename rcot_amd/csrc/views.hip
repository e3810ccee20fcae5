// Views of an image and their weighted blend: the two device steps of tiled and self-ensemble inference (rcot_amd/tiles.py,
// rcot_amd.tester --tile / --tile_window / --tile_batch / --ensemble).
//   rcot_view_gather : image [planes][H][W] -> nm * ny * nx views, view (k, iy, ix) = data_augmentation(window (iy, ix), modes[k])
//   rcot_view_blend  : the views (after the network) -> image: every pixel is the weighted mean of the view elements that the maps
//                      placed on it, summed in ascending view order (include/rcot_hip.h states the arithmetic).
// Both move each byte once and are memory-bound.  A workgroup of 256 threads owns a 32 x 32 tile of WINDOW pixels (gather) or of
// IMAGE pixels (blend) and touches the image side as float4 row pieces.  The view side of modes 0, 1, 4, 5 is a float4 row piece as
// well (reversed in the register for the mirrored ones).  Modes 2, 3, 6, 7 transpose: a row piece of the window is a column piece of
// the view, so the tile goes through a 32 x 33 LDS tile and the view side is touched by the thread that owns four consecutive ROWS
// of one window column — a float4 row piece of the view again.  Neither global side is strided in any mode.
// The origins and modes travel in the kernel's argument block (ViewGeom): no device table, no copy before the launch.
#include "common.h"
#include "../../include/rcot_hip.h"

namespace {

constexpr int VIEW_MAX_ORIGINS = 64;   // per axis: what the argument block holds
constexpr int TS = 32;                 // tile side; 256 threads = 32 rows x 8 float4

struct ViewGeom {
    int ys[VIEW_MAX_ORIGINS], xs[VIEW_MAX_ORIGINS], modes[8];
    int ny, nx, nm, Th, Tw, H, W, planes;
};

__device__ __forceinline__ float4 reversed(float4 a) { return make_float4(a.w, a.z, a.y, a.x); }

// Where the four window pixels (sy, sx .. sx + 3) [along_rows = false] or (sy .. sy + 3, sx) [true] lie in the Rv x Cv view of `mode`:
// always four consecutive elements of one view row.  Returns the offset of the lowest and whether they run backwards.
__device__ __forceinline__ long view_piece(int inv, int Rv, int Cv, int sy, int sx, bool along_rows, bool& backwards) {
    int i0, j0, i1, j1;
    rcot::dihedral(inv, Rv, Cv, sy, sx, i0, j0);
    rcot::dihedral(inv, Rv, Cv, along_rows ? sy + 3 : sy, along_rows ? sx : sx + 3, i1, j1);
    backwards = j1 < j0;
    return (long)i0 * Cv + (backwards ? j1 : j0);
}

// grid: x = 32 x 32 tiles of one window, y = view, z = planes (strided)
__global__ __launch_bounds__(256) void view_gather_kernel(const float* __restrict__ img, float* __restrict__ views, const ViewGeom g) {
    __shared__ float s[TS][TS + 1];
    const int tiles_x = (g.Tw + TS - 1) / TS;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int v = blockIdx.y;
    const int ix = v % g.nx, iy = (v / g.nx) % g.ny, k = v / (g.nx * g.ny);
    const int mode = g.modes[k], inv = rcot::dihedral_inverse(mode);
    const bool tr = (mode & 2) != 0;
    const int Rv = tr ? g.Tw : g.Th, Cv = tr ? g.Th : g.Tw;
    const int r = threadIdx.x >> 3, q = threadIdx.x & 7;
    const int sy = ty * TS + r, sx = tx * TS + 4 * q;                  // this thread's row piece of the window
    const bool in = sy < g.Th && sx < g.Tw;
    const int cy = ty * TS + 4 * q, cx = tx * TS + r;                  // and its column piece (transposing modes)
    const bool cin = cy < g.Th && cx < g.Tw;
    const long plane = (long)g.H * g.W, vplane = (long)g.Th * g.Tw;
    const long src_off = (long)(g.ys[iy] + sy) * g.W + g.xs[ix] + sx;
    bool back = false;
    const long dst_off = tr ? (cin ? view_piece(inv, Rv, Cv, cy, cx, true, back) : 0) : (in ? view_piece(inv, Rv, Cv, sy, sx, false, back) : 0);
    for (int c = blockIdx.z; c < g.planes; c += gridDim.z) {
        float* dst = views + ((long)v * g.planes + c) * vplane;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in) a = *reinterpret_cast<const float4*>(img + c * plane + src_off);
        if (!tr) {
            if (in) *reinterpret_cast<float4*>(dst + dst_off) = back ? reversed(a) : a;
        } else {
            s[r][4 * q + 0] = a.x; s[r][4 * q + 1] = a.y; s[r][4 * q + 2] = a.z; s[r][4 * q + 3] = a.w;
            __syncthreads();
            if (cin) {
                const float4 b = make_float4(s[4 * q + 0][r], s[4 * q + 1][r], s[4 * q + 2][r], s[4 * q + 3][r]);
                *reinterpret_cast<float4*>(dst + dst_off) = back ? reversed(b) : b;
            }
            __syncthreads();
        }
    }
}

// grid: x = 32 x 32 tiles of the image, z = planes (strided)
__global__ __launch_bounds__(256) void view_blend_kernel(const float* __restrict__ views, const float* __restrict__ wy,
                                                         const float* __restrict__ wx, float* __restrict__ out, const ViewGeom g) {
    __shared__ float s[TS][TS + 1];
    const int tiles_x = (g.W + TS - 1) / TS;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int Y0 = ty * TS, X0 = tx * TS;
    // the windows that reach this tile: one contiguous range per axis (sorted origins, one size), found once per workgroup
    int iy_lo = 0, ix_lo = 0;
    while (iy_lo < g.ny && g.ys[iy_lo] + g.Th <= Y0) ++iy_lo;
    while (ix_lo < g.nx && g.xs[ix_lo] + g.Tw <= X0) ++ix_lo;
    int iy_hi = iy_lo, ix_hi = ix_lo;
    while (iy_hi < g.ny && g.ys[iy_hi] < Y0 + TS) ++iy_hi;
    while (ix_hi < g.nx && g.xs[ix_hi] < X0 + TS) ++ix_hi;
    const int r = threadIdx.x >> 3, q = threadIdx.x & 7;
    const int y = Y0 + r, x = X0 + 4 * q;                              // this thread's row piece of the image
    const bool active = y < g.H && x < g.W;
    const long plane = (long)g.H * g.W, vplane = (long)g.Th * g.Tw;
    for (int c = blockIdx.z; c < g.planes; c += gridDim.z) {
        float4 num = make_float4(0.f, 0.f, 0.f, 0.f), den = num;
        for (int k = 0; k < g.nm; ++k) {
            const int mode = g.modes[k], inv = rcot::dihedral_inverse(mode);
            const bool tr = (mode & 2) != 0;
            const int Rv = tr ? g.Tw : g.Th, Cv = tr ? g.Th : g.Tw;
            for (int iy = iy_lo; iy < iy_hi; ++iy) {
                const int sy = y - g.ys[iy];
                const bool cov_y = active && sy >= 0 && sy < g.Th;
                for (int ix = ix_lo; ix < ix_hi; ++ix) {
                    const int sx = x - g.xs[ix];
                    const bool cov = cov_y && sx >= 0 && sx < g.Tw;
                    const float* vp = views + (((long)(k * g.ny + iy) * g.nx + ix) * g.planes + c) * vplane;
                    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                    bool back;
                    if (!tr) {
                        if (cov) {
                            a = *reinterpret_cast<const float4*>(vp + view_piece(inv, Rv, Cv, sy, sx, false, back));
                            if (back) a = reversed(a);
                        }
                    } else {
                        const int cy = Y0 - g.ys[iy] + 4 * q, cx = X0 - g.xs[ix] + r;      // column piece: rows cy .. cy + 3 of window column cx
                        if (cy >= 0 && cy < g.Th && cx >= 0 && cx < g.Tw) {
                            float4 b = *reinterpret_cast<const float4*>(vp + view_piece(inv, Rv, Cv, cy, cx, true, back));
                            if (back) b = reversed(b);
                            s[4 * q + 0][r] = b.x; s[4 * q + 1][r] = b.y; s[4 * q + 2][r] = b.z; s[4 * q + 3][r] = b.w;
                        }
                        __syncthreads();
                        if (cov) a = make_float4(s[r][4 * q + 0], s[r][4 * q + 1], s[r][4 * q + 2], s[r][4 * q + 3]);
                        __syncthreads();
                    }
                    if (cov) {
                        float4 w = make_float4(1.f, 1.f, 1.f, 1.f);
                        if (wy) {
                            const float wr = wy[sy];
                            const float4 wc = *reinterpret_cast<const float4*>(wx + sx);
                            w = make_float4(__fmul_rn(wr, wc.x), __fmul_rn(wr, wc.y), __fmul_rn(wr, wc.z), __fmul_rn(wr, wc.w));
                        }
                        num.x = __fadd_rn(num.x, __fmul_rn(w.x, a.x)); den.x = __fadd_rn(den.x, w.x);
                        num.y = __fadd_rn(num.y, __fmul_rn(w.y, a.y)); den.y = __fadd_rn(den.y, w.y);
                        num.z = __fadd_rn(num.z, __fmul_rn(w.z, a.z)); den.z = __fadd_rn(den.z, w.z);
                        num.w = __fadd_rn(num.w, __fmul_rn(w.w, a.w)); den.w = __fadd_rn(den.w, w.w);
                    }
                }
            }
        }
        if (active)
            *reinterpret_cast<float4*>(out + c * plane + (long)y * g.W + x) =
                make_float4(__fdiv_rn(num.x, den.x), __fdiv_rn(num.y, den.y), __fdiv_rn(num.z, den.z), __fdiv_rn(num.w, den.w));
    }
}

// one axis of windows: sorted multiples of 4 from 0, no gap, the last one ending at the image's edge
bool axis_ok(const int* o, int n, int T, int L) {
    if (o[0] != 0 || (long)o[n - 1] + T != L) return false;
    for (int i = 0; i < n; ++i) {
        if (o[i] < 0 || (o[i] & 3)) return false;
        if (i + 1 < n && (o[i + 1] <= o[i] || (long)o[i + 1] - o[i] > T)) return false;
    }
    return true;
}

// the refusals both entry points share (include/rcot_hip.h); fills the argument block
int view_geometry(int planes, int H, int W, const int* ys, int ny, const int* xs, int nx, const int* modes, int nm, int Th, int Tw,
                  ViewGeom& g) {
    if (!ys || !xs || !modes || planes < 1 || ny < 1 || nx < 1 || nm < 1 || nm > 8) return RCOT_EINVAL;   // 9 modes repeat one
    if (Th < 4 || Tw < 4 || (Th & 3) || (Tw & 3) || H < 4 || W < 4 || (H & 3) || (W & 3)) return RCOT_EINVAL;
    unsigned seen = 0;
    for (int k = 0; k < nm; ++k) {
        if (modes[k] < 0 || modes[k] > 7 || (seen >> modes[k] & 1u)) return RCOT_EINVAL;
        seen |= 1u << modes[k];
    }
    if (ny > VIEW_MAX_ORIGINS || nx > VIEW_MAX_ORIGINS) return RCOT_EUNSUPPORTED;
    if (!axis_ok(ys, ny, Th, H) || !axis_ok(xs, nx, Tw, W)) return RCOT_EINVAL;
    for (int i = 0; i < ny; ++i) g.ys[i] = ys[i];
    for (int i = 0; i < nx; ++i) g.xs[i] = xs[i];
    for (int k = 0; k < nm; ++k) g.modes[k] = modes[k];
    g.ny = ny; g.nx = nx; g.nm = nm; g.Th = Th; g.Tw = Tw; g.H = H; g.W = W; g.planes = planes;
    return RCOT_OK;
}

}  // namespace

extern "C" int rcot_view_gather(const float* img, int planes, int H, int W, const int* ys, int ny, const int* xs, int nx,
                                const int* modes, int nm, int Th, int Tw, float* views, void* stream) {
    if (!img || !views || !rcot::al16(img) || !rcot::al16(views)) return RCOT_EINVAL;
    ViewGeom g = {};
    const int rc = view_geometry(planes, H, W, ys, ny, xs, nx, modes, nm, Th, Tw, g);
    if (rc != RCOT_OK) return rc;
    const dim3 grid(rcot::cdiv(Th, TS) * rcot::cdiv(Tw, TS), nm * ny * nx, planes < 65535 ? planes : 65535);
    RCOT_LAUNCH(view_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, img, views, g);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

extern "C" int rcot_view_blend(const float* views, int planes, int H, int W, const int* ys, int ny, const int* xs, int nx,
                               const int* modes, int nm, int Th, int Tw, const float* wy, const float* wx, float* out, void* stream) {
    if (!views || !out || !rcot::al16(views) || !rcot::al16(out)) return RCOT_EINVAL;
    if ((wy == nullptr) != (wx == nullptr) || !rcot::al16(wy) || !rcot::al16(wx)) return RCOT_EINVAL;
    ViewGeom g = {};
    const int rc = view_geometry(planes, H, W, ys, ny, xs, nx, modes, nm, Th, Tw, g);
    if (rc != RCOT_OK) return rc;
    const dim3 grid(rcot::cdiv(H, TS) * rcot::cdiv(W, TS), 1, planes < 65535 ? planes : 65535);
    RCOT_LAUNCH(view_blend_kernel, grid, dim3(256), 0, (hipStream_t)stream, views, wy, wx, out, g);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}
