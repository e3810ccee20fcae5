// Fused flat-buffer optimizers (reference: torch.optim.RMSprop / Adam defaults, trainer.py:121-126).
// Parameters, gradients and state of one network live in contiguous fp32 buffers, so one launch
// updates the whole network at HBM speed (5 streams of 4 B per element for RMSprop).
#include "common.h"
#include "../../include/rcot_hip.h"

namespace {

using rcot::al16;

// ---- the optimizer steps: ONE kernel, a rule (what happens to one element) x a source (where the launch's scalars come from) ----
// What may change from one iteration to the next.  lr: RMSprop's rate; for Adam the step size lr / (1 - b1^t).  rsqrt_bc2: 1 / sqrt(1 - b2^t).
// gscale: the factor on the gradient (a loss scale, or the clipping decision).  nlrwd: AdamW's -(float)(lr wd), the product formed in double.
struct StepScalars {
    float lr, rsqrt_bc2, gscale, nlrwd;
};

// The rules: hyper-parameters that never change, the number of state buffers, and what happens to one element: decay() (AdamW's alone
// does something), then the update — one expression each, so that a guarded step with scale 1 is the same arithmetic as the plain one.
struct RmsProp {
    static constexpr int kStates = 1;
    static constexpr bool kAdam = false, kDecay = false;
    float alpha, oma, eps;
    __device__ __forceinline__ void decay(float&, const StepScalars&) const {}
    __device__ __forceinline__ void operator()(float& p, float g, float& s, float&, const StepScalars& k) const {
        const float gg = g * k.gscale;
        s = alpha * s + oma * gg * gg;
        p -= k.lr * gg / (sqrtf(s) + eps);
    }
};

// AdamW (torch.optim.AdamW): decoupled weight decay p <- p - (lr wd) p before Adam's update, as one fused multiply-add in the increment
// form.  The factor form (float)(1 - lr wd) would round 1 - 3e-8 (lr 3e-4, wd 1e-4) to 1 - 2^-24: twice the decay asked for.  Adam's
// bytes, plus one FMA per element.
template <bool Decay>
struct AdamRule {
    static constexpr int kStates = 2;
    static constexpr bool kAdam = true, kDecay = Decay;
    float b1, b2, omb1, omb2, eps;
    __device__ __forceinline__ void decay(float& p, const StepScalars& k) const {
        if constexpr (Decay) p = __builtin_fmaf(k.nlrwd, p, p);
    }
    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v, const StepScalars& k) const {
        const float gg = g * k.gscale;
        m = b1 * m + omb1 * gg;
        v = b2 * v + omb2 * gg * gg;
        p -= k.lr * m / (sqrtf(v) * k.rsqrt_bc2 + eps);
    }
};
using Adam = AdamRule<false>;
using AdamW = AdamRule<true>;

// The sources.  read() fills what the rule uses and says whether the launch does anything.
struct ByValue {
    StepScalars k;
    template <class Rule> __device__ __forceinline__ bool read(StepScalars& o) const {
        o = k;
        return true;
    }
};

// The control block (uniform loads of words that the decision launch, the host or the schedule's advance launch wrote).  A skipped step
// says no before anything is loaded: p and the state stay bit for bit what they were.  counter: which of the block's two Adam step
// counts this range follows; a count of 0 (no taken decision has advanced it) has no bias correction, and the launch does nothing.
// lr wd is formed here, in double, from the block's learning rate.
struct FromCtrl {
    const double* ctrl;
    int counter;
    double wd;
    template <class Rule> __device__ __forceinline__ bool read(StepScalars& o) const {
        const long long* ci = reinterpret_cast<const long long*>(ctrl);
        if (ci[RCOT_CB_SKIP]) return false;
        if constexpr (Rule::kAdam) {
            if (ci[RCOT_CB_T + counter] <= 0) return false;
            o.lr = (float)(ctrl[RCOT_CB_LR] / ctrl[RCOT_CB_BC1 + counter]);
            o.rsqrt_bc2 = (float)(1.0 / sqrt(ctrl[RCOT_CB_BC2 + counter]));
        } else {
            o.lr = (float)ctrl[RCOT_CB_LR];
        }
        o.gscale = (float)ctrl[RCOT_CB_SCALE];
        if constexpr (Rule::kDecay) o.nlrwd = -(float)(ctrl[RCOT_CB_LR] * wd);
        return true;
    }
};

// s1: the second state buffer of a rule that has one (never touched otherwise)
template <class Rule, class Src>
__global__ __launch_bounds__(256) void step_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ s0,
                                                   float4* __restrict__ s1, long n4, Rule rule, Src src) {
    StepScalars k{};
    if (!src.template read<Rule>(k)) return;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 pv = p[i], gv = g[i], av = s0[i], bv{};
        if constexpr (Rule::kStates == 2) bv = s1[i];
        rule.decay(pv.x, k);                     // (all four before the first update: the loop's schedule follows the statement order)
        rule.decay(pv.y, k);
        rule.decay(pv.z, k);
        rule.decay(pv.w, k);
        rule(pv.x, gv.x, av.x, bv.x, k);
        rule(pv.y, gv.y, av.y, bv.y, k);
        rule(pv.z, gv.z, av.z, bv.z, k);
        rule(pv.w, gv.w, av.w, bv.w, k);
        p[i] = pv;
        s0[i] = av;
        if constexpr (Rule::kStates == 2) s1[i] = bv;
    }
}

// Weight average: ema += omd * (p - ema), one fused multiply-add per element (3 streams of 4 B per element).  The increment form keeps
// p - ema exact (or nearly so) where the two are close, which is what an fp32 average at decay 0.999 rests on.
// vec: n4 float4 elements grid-stride, then the n - 4 n4 <= 3 tail elements by the first lanes of workgroup 0; else n scalars.
__device__ __forceinline__ float ema_one(float e, float pv, float omd) { return __builtin_fmaf(omd, pv - e, e); }

__device__ __forceinline__ void ema_body(float* __restrict__ ema, const float* __restrict__ p, long n, float omd, int vec) {
    const long t0 = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    if (vec) {
        float4* __restrict__ e4 = (float4*)ema;
        const float4* __restrict__ p4 = (const float4*)p;
        const long n4 = n >> 2;
        for (long i = t0; i < n4; i += stride) {
            float4 ev = e4[i];
            const float4 pv = p4[i];
            ev.x = ema_one(ev.x, pv.x, omd);
            ev.y = ema_one(ev.y, pv.y, omd);
            ev.z = ema_one(ev.z, pv.z, omd);
            ev.w = ema_one(ev.w, pv.w, omd);
            e4[i] = ev;
        }
        const long i = (n4 << 2) + t0;
        if (t0 < 3 && i < n) ema[i] = ema_one(ema[i], p[i], omd);
    } else {
        for (long i = t0; i < n; i += stride) ema[i] = ema_one(ema[i], p[i], omd);
    }
}

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float omd, int vec) {
    ema_body(ema, p, n, omd, vec);
}

// The same body with 1 - decay read from a device word (a uniform load of what an earlier rcot_sched_advance launch wrote): the decay of
// an EMA warm-up changes every iteration, and a recorded launch carries no by-value argument that does.
__global__ __launch_bounds__(256) void ema_dev_kernel(float* __restrict__ ema, const float* __restrict__ p, long n,
                                                      const double* __restrict__ omd_word, int vec) {
    ema_body(ema, p, n, (float)*omd_word, vec);
}

// ---- gradient-norm clipping and non-finite step skip, decided on the device (control block: include/rcot_hip.h, RCOT_CB_*) ----
// Three launches per guarded step: sumsq_kernel (one read of the gradients, 4 B per element: one fp64 partial per workgroup), decide_kernel
// (ONE workgroup: the partials in a fixed order, the rule, the counters) and a guarded step kernel that reads the decision.  Every word a
// kernel reads was written by an EARLIER launch or by the host: no workgroup reads what another workgroup of its launch writes.
__device__ __forceinline__ double sq4(double a, const float4 v) {
    a = fma((double)v.x, (double)v.x, a);
    a = fma((double)v.y, (double)v.y, a);
    a = fma((double)v.z, (double)v.z, a);
    return fma((double)v.w, (double)v.w, a);
}

// head: the 0 .. 3 elements before the first 16-byte boundary of g (host-computed; <= n).  Then n4 float4 elements grid-stride, four
// independent loads in flight per lane, then the tail; head and tail (at most 3 + 3 elements) by the first six lanes of workgroup 0.
// fp64 throughout: the square of an fp32 value is exact in fp64 and the kernel is bound by HBM.
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long n, int head, double* __restrict__ partials) {
    __shared__ double red[4];
    const long t0 = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    const float4* __restrict__ g4 = (const float4*)(g + head);
    const long n4 = (n - head) >> 2;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    long i = t0;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const float4 v0 = g4[i], v1 = g4[i + stride], v2 = g4[i + 2 * stride], v3 = g4[i + 3 * stride];
        a0 = sq4(a0, v0);
        a1 = sq4(a1, v1);
        a2 = sq4(a2, v2);
        a3 = sq4(a3, v3);
    }
    for (; i < n4; i += stride) a0 = sq4(a0, g4[i]);
    if (t0 < 6) {
        const long j = t0 < 3 ? t0 : (long)head + (n4 << 2) + (t0 - 3);
        if (t0 < 3 ? t0 < head : j < n) {
            const double x = (double)g[j];
            a1 = fma(x, x, a1);
        }
    }
    double s = (a0 + a1) + (a2 + a3);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup.  total = the partials in a fixed order (strided per-thread sums, then a tree); norm, scale and skip by the rule of
// torch.nn.utils.clip_grad_norm_ / GradScaler; counters; for Adam the step counts named by flags (bit k = RCOT_DECIDE_ADAM0 << k: counter k) advance when the
// step is taken, and their bias corrections 1 - beta^t are left in the block for the guarded step launches.
__global__ __launch_bounds__(256) void decide_kernel(const double* __restrict__ partials, int nparts, double* __restrict__ ctrl, int flags,
                                                     double b1, double b2) {
    __shared__ double sd[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int b = t; b < nparts; b += 256) s += partials[b];
    sd[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sd[t] += sd[t + o];
        __syncthreads();
    }
    if (t != 0) return;
    long long* ci = reinterpret_cast<long long*>(ctrl);
    const double total = sd[0];
    // RCOT_DECIDE_INHERIT: a later step on the same batch (the gradient penalty after the critic step).  When the block's previous decision
    // skipped, this one skips too, whatever its own sum: the flag read here was written by an earlier launch.
    const bool inherited = (flags & RCOT_DECIDE_INHERIT) && ci[RCOT_CB_SKIP] != 0;
    const bool skip = inherited || !isfinite(total);
    const double norm = sqrt(total);
    const double scale = skip ? 0.0 : fmin(1.0, ctrl[RCOT_CB_MAX_NORM] / (norm + 1e-6));
    ctrl[RCOT_CB_NORM] = norm;
    ctrl[RCOT_CB_SCALE] = scale;
    ci[RCOT_CB_SKIP] = skip ? 1 : 0;
    ci[RCOT_CB_STEPS] += 1;
    if (skip) {
        ci[RCOT_CB_SKIPPED] += 1;
        return;
    }
    if (scale < 1.0) ci[RCOT_CB_CLIPPED] += 1;
    if (norm > ctrl[RCOT_CB_MAX_SEEN]) ctrl[RCOT_CB_MAX_SEEN] = norm;
    for (int k = 0; k < 2; ++k) {
        if (!(flags >> k & 1)) continue;
        const long long tk = ci[RCOT_CB_T + k] + 1;
        ci[RCOT_CB_T + k] = tk;
        ctrl[RCOT_CB_BC1 + k] = 1.0 - pow(b1, (double)tk);
        ctrl[RCOT_CB_BC2 + k] = 1.0 - pow(b2, (double)tk);
    }
}

// ---- per-iteration schedules held on the device (schedule block: include/rcot_hip.h, RCOT_SB_*) ----
// ONE workgroup, one lane of it: the iteration's rate from the table into the block and into up to two destination words (the
// RCOT_CB_LR words of the two optimizers), the counter, and the 1 - D_u of the EMA warm-up.  Every word written here is read by LATER
// launches only.  Plain stores of doubles and 64-bit integers.
__global__ __launch_bounds__(64) void sched_advance_kernel(double* __restrict__ sched, const double* __restrict__ table, int n_table,
                                                           double* lr_dst0, double mult0, double* lr_dst1, double mult1) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long* si = reinterpret_cast<long long*>(sched);
    if (table) {
        const long long t = si[RCOT_SB_T];
        long long idx = t < (long long)n_table - 1 ? t : (long long)n_table - 1;      // past the end the last entry holds
        if (idx < 0) idx = 0;
        const double v = table[idx];
        if (lr_dst0) *lr_dst0 = v * mult0;
        if (lr_dst1) *lr_dst1 = v * mult1;
        sched[RCOT_SB_LR] = v;
        si[RCOT_SB_T] = t + 1;
    }
    const double D = sched[RCOT_SB_EMA_DECAY];
    if (D > 0.0) {
        const long long u = si[RCOT_SB_EMA_UPDATES];
        const double w = (1.0 + (double)u) / (10.0 + (double)u);
        sched[RCOT_SB_EMA_OMD] = 1.0 - (D < w ? D : w);
        si[RCOT_SB_EMA_UPDATES] = u + 1;
    }
}

// What every step entry point refuses alike (null, n <= 0 or no multiple of 4, a buffer off a 16-byte boundary), else the launch: one
// float4 per lane, at most 4096 workgroups.  s1 is looked at only for a rule with two state buffers.
template <class Rule, class Src>
inline int launch_step(float* p, const float* g, float* s0, float* s1, long n, const Rule& rule, const Src& src, void* stream) {
    if (!p || !g || !s0 || n <= 0 || (n & 3) || !al16(p) || !al16(g) || !al16(s0) || (Rule::kStates == 2 && (!s1 || !al16(s1))))
        return RCOT_EINVAL;
    const long n4 = n >> 2;
    long grid = (n4 + 255) / 256;
    if (grid > 4096) grid = 4096;
    RCOT_LAUNCH((step_kernel<Rule, Src>), dim3((int)grid), dim3(256), 0, (hipStream_t)stream, (float4*)p, (const float4*)g, (float4*)s0,
                (float4*)s1, n4, rule, src);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

inline RmsProp rmsprop_rule(double alpha, double eps) { return {(float)alpha, (float)(1.0 - alpha), (float)eps}; }
template <class Rule> inline Rule adam_rule(double b1, double b2, double eps) {
    return {(float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)eps};
}
// Adam's by-value scalars of step `step` >= 1: the bias corrections in double, as torch.optim forms them on the host
inline ByValue adam_by_value(double lr, double b1, double b2, int step, double grad_scale, double weight_decay) {
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    return {{(float)(lr / bc1), (float)(1.0 / sqrt(bc2)), (float)grad_scale, -(float)(lr * weight_decay)}};
}
inline bool ctrl_ok(const double* ctrl, int counter) { return ctrl && !(reinterpret_cast<uintptr_t>(ctrl) & 7) && counter >= 0 && counter <= 1; }

// what rcot_ema_step and rcot_ema_step_dev refuse alike (false), else the form (float4 body + tail, or scalar) and the grid
inline bool ema_geometry(const float* ema, const float* p, long n, int* vec, long* grid) {
    if (!ema || !p || n <= 0) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(ema), b = reinterpret_cast<uintptr_t>(p);
    if ((a & 3) || (b & 3)) return false;
    const uintptr_t bytes = (uintptr_t)n * 4;
    if (a < b + bytes && b < a + bytes) return false;                     // the ranges overlap
    *vec = al16(ema) && al16(p);
    const long items = *vec ? (n >> 2) : n;
    long g = (items + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;                                                     // n < 4 on the float4 path: the tail alone
    *grid = g;
    return true;
}
}  // namespace

extern "C" {

// Hyper-parameters arrive as doubles so that 1-alpha / 1-beta / bias corrections are formed in double
// precision exactly as torch.optim does on the host (1 - 0.999f would be off by 1.3e-5 relative).
int rcot_rmsprop_step(float* p, const float* g, float* sq, long n, double lr, double alpha, double eps,
                      double grad_scale, void* stream) {
    return launch_step(p, g, sq, nullptr, n, rmsprop_rule(alpha, eps), ByValue{{(float)lr, 0.f, (float)grad_scale, 0.f}}, stream);
}

int rcot_adam_step(float* p, const float* g, float* m, float* v, long n, double lr, double b1, double b2, double eps,
                   int step, double grad_scale, void* stream) {
    if (step <= 0) return RCOT_EINVAL;
    return launch_step(p, g, m, v, n, adam_rule<Adam>(b1, b2, eps), adam_by_value(lr, b1, b2, step, grad_scale, 0.0), stream);
}

// 1 - decay is formed in double, as 1 - alpha above.  Any n >= 1 and any 4-byte-aligned pointers: float4 accesses when both are
// 16-byte aligned, a scalar grid-stride sweep otherwise.  !(0 <= decay < 1) also refuses NaN.
int rcot_ema_step(float* ema, const float* p, long n, double decay, void* stream) {
    if (!(decay >= 0.0 && decay < 1.0)) return RCOT_EINVAL;
    int vec;
    long grid;
    if (!ema_geometry(ema, p, n, &vec, &grid)) return RCOT_EINVAL;
    RCOT_LAUNCH(ema_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, ema, p, n, (float)(1.0 - decay), vec);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

// rcot_ema_step with omd = (float)*omd_word read on the device: the same refusals and the same three forms.
int rcot_ema_step_dev(float* ema, const float* p, long n, const double* omd_word, void* stream) {
    if (!omd_word || (reinterpret_cast<uintptr_t>(omd_word) & 7)) return RCOT_EINVAL;
    int vec;
    long grid;
    if (!ema_geometry(ema, p, n, &vec, &grid)) return RCOT_EINVAL;
    RCOT_LAUNCH(ema_dev_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, ema, p, n, omd_word, vec);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_adamw_step(float* p, const float* g, float* m, float* v, long n, double lr, double b1, double b2, double eps, int step,
                    double grad_scale, double weight_decay, void* stream) {
    if (!(weight_decay >= 0.0)) return RCOT_EINVAL;                        // refuses NaN too
    if (weight_decay == 0.0) return rcot_adam_step(p, g, m, v, n, lr, b1, b2, eps, step, grad_scale, stream);
    if (step <= 0) return RCOT_EINVAL;
    return launch_step(p, g, m, v, n, adam_rule<AdamW>(b1, b2, eps), adam_by_value(lr, b1, b2, step, grad_scale, weight_decay), stream);
}

int rcot_sched_advance(double* sched, const double* table, int n_table, double* lr_dst0, double mult0, double* lr_dst1, double mult1,
                       void* stream) {
    if (!sched || (reinterpret_cast<uintptr_t>(sched) & 7) || (table && n_table <= 0) || (reinterpret_cast<uintptr_t>(table) & 7) ||
        (reinterpret_cast<uintptr_t>(lr_dst0) & 7) || (reinterpret_cast<uintptr_t>(lr_dst1) & 7))
        return RCOT_EINVAL;
    RCOT_LAUNCH(sched_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sched, table, n_table, lr_dst0, mult0, lr_dst1, mult1);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

// ---- the guarded step (rcot_hip.h): rcot_grad_sumsq -> rcot_grad_decide -> rcot_rmsprop_step_guarded | rcot_adam_step_guarded
int rcot_grad_sumsq_parts(long n) {
    if (n <= 0) return 0;
    const long g = ((n >> 2) + 255) / 256;
    return (int)(g > RCOT_SUMSQ_MAX_PARTS ? RCOT_SUMSQ_MAX_PARTS : g < 1 ? 1 : g);
}

int rcot_grad_sumsq(const float* g, long n, double* partials, void* stream) {
    if (!g || !partials || n <= 0 || (reinterpret_cast<uintptr_t>(g) & 3) || (reinterpret_cast<uintptr_t>(partials) & 7)) return RCOT_EINVAL;
    long head = (long)(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2);   // elements before the first 16-byte boundary
    if (head > n) head = n;
    RCOT_LAUNCH(sumsq_kernel, dim3(rcot_grad_sumsq_parts(n)), dim3(256), 0, (hipStream_t)stream, g, n, (int)head, partials);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_grad_decide(const double* partials, int nparts, double* ctrl, int flags, double b1, double b2, void* stream) {
    if (!partials || !ctrl || nparts <= 0 || nparts > RCOT_SUMSQ_MAX_PARTS || (flags & ~7) || (reinterpret_cast<uintptr_t>(partials) & 7) ||
        (reinterpret_cast<uintptr_t>(ctrl) & 7))
        return RCOT_EINVAL;
    RCOT_LAUNCH(decide_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nparts, ctrl, flags, b1, b2);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_rmsprop_step_guarded(float* p, const float* g, float* sq, long n, double alpha, double eps, const double* ctrl, void* stream) {
    if (!ctrl_ok(ctrl, 0)) return RCOT_EINVAL;
    return launch_step(p, g, sq, nullptr, n, rmsprop_rule(alpha, eps), FromCtrl{ctrl, 0, 0.0}, stream);
}

int rcot_adam_step_guarded(float* p, const float* g, float* m, float* v, long n, double b1, double b2, double eps, const double* ctrl,
                           int counter, void* stream) {
    if (!ctrl_ok(ctrl, counter)) return RCOT_EINVAL;
    return launch_step(p, g, m, v, n, adam_rule<Adam>(b1, b2, eps), FromCtrl{ctrl, counter, 0.0}, stream);
}

int rcot_adamw_step_guarded(float* p, const float* g, float* m, float* v, long n, double b1, double b2, double eps, const double* ctrl,
                            int counter, double weight_decay, void* stream) {
    if (!(weight_decay >= 0.0)) return RCOT_EINVAL;
    if (weight_decay == 0.0) return rcot_adam_step_guarded(p, g, m, v, n, b1, b2, eps, ctrl, counter, stream);
    if (!ctrl_ok(ctrl, counter)) return RCOT_EINVAL;
    return launch_step(p, g, m, v, n, adam_rule<AdamW>(b1, b2, eps), FromCtrl{ctrl, counter, weight_decay}, stream);
}

}  // extern "C"
