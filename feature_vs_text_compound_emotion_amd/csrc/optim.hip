// optim.hip -- the optimiser update and the feature-to-frame row gather of the host loop.
//
// sgd_nesterov_flat: the reference trains with torch.optim.SGD(momentum=0.9, nesterov=True, weight_decay=1e-4)
// (/root/reference/instantiators.py:74-92, trainer.py:385-391).  All trainable parameters, their gradients and the
// momentum buffers live in three flat fp32 buffers (data_parallel.py), so the whole update is ONE bandwidth-bound
// launch (16 B read + 8 B written per parameter) instead of ~100 multi-tensor launches.  Arithmetic follows torch's
// _single_tensor_sgd operation by operation (grad + wd*p; buf = mu*buf + (1-damp)*d, or d on the first step;
// d + mu*buf; p - lr*d) so the result is bit-identical to it.
//
// adam_flat: the reference's other optimiser, torch.optim.Adam(betas, eps, weight_decay, amsgrad) with L2 weight decay
// (instantiators.py:81-92), as ONE launch over the same flat buffers plus the moment buffers (20 B read + 12 B written
// per parameter, 28 B + 8 B with AMSGrad) instead of torch's ~10 multi-tensor passes.  Per element it follows the
// non-capturable branch of torch's _multi_tensor_adam operation by operation; the step-dependent terms
// step_size = -lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) are computed on the host in double as torch does.
//
// *_amp: the same two updates driven by torch.amp.GradScaler without a host read (the optimisers declare
// _step_supports_amp_scaling): grad_scale and found_inf arrive as device scalars, a launch with found_inf != 0 changes
// nothing (parameters, moments, step count), otherwise the bucket is unscaled in the same pass.  The applied-step count lives
// on the device (SGD's first-step rule, Adam's bias corrections through a host-built table indexed by it).
// amp_check_unscale_flat is the bucket form of torch._amp_foreach_non_finite_check_and_unscale_ (one launch instead of one
// foreach chain over hundreds of per-parameter views).
//
// gather_rows: out[i] = src[index[i]] (zeros for index < 0): token -> frame spreading of the BERT features
// (abaw5_pre_processing/base/speech.py:690-738) and the edge-padded frame indexing of VGGish rows
// (base/preprocessing.py:992-1018); the index plan is host logic (feature_extractor.py).
#include <stdint.h>

#include <cmath>

#include "cer_internal.h"

namespace cer {

// torch's _single_tensor_sgd on one float4 of the flat buffers (shared by the plain and the loss-scaled update)
__device__ __forceinline__ void sgd_update4(float4 &pv, const float4 &gv, float4 &bv, float lr, float mu, float damp, float wd,
                                            int nesterov, int first) {
    float *pp = reinterpret_cast<float *>(&pv), *bb = reinterpret_cast<float *>(&bv);
    const float *gg = reinterpret_cast<const float *>(&gv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float d = wd != 0.f ? __fmaf_rn(wd, pp[e], gg[e]) : gg[e];          // grad.add(param, alpha=wd)
        if (mu != 0.f) {
            bb[e] = first ? d : __fmaf_rn(1.f - damp, d, __fmul_rn(mu, bb[e]));  // buf.mul_(mu).add_(d, alpha=1-damp)
            d = nesterov ? __fmaf_rn(mu, bb[e], d) : bb[e];                  // d.add(buf, alpha=mu)
        }
        pp[e] = __fmaf_rn(-lr, d, pp[e]);                                    // param.add_(d, alpha=-lr)
    }
}

__global__ void sgd_nesterov_flat_kernel(float4 *__restrict__ p, const float4 *__restrict__ g, float4 *__restrict__ buf,
                                         size_t n4, float lr, float mu, float damp, float wd, int nesterov, int first) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 pv = p[i];
    const float4 gv = g[i];
    float4 bv = first ? make_float4(0, 0, 0, 0) : buf[i];
    sgd_update4(pv, gv, bv, lr, mu, damp, wd, nesterov, first);
    p[i] = pv;
    if (mu != 0.f) buf[i] = bv;
}

// sqrtf and '/' are correctly rounded here (no fast-math; HIP's default -fhip-fp32-correctly-rounded-divide-sqrt); the
// __f*_rn intrinsics spell out every other rounding so no contraction can change the result.
__device__ __forceinline__ void adam_update4(float4 &pv, const float4 &gv, float4 &mv, float4 &vv, float4 &xv, bool amsgrad,
                                             float one_m_b1, float b2, float one_m_b2, float eps, float wd, float step_size,
                                             float bc2_sqrt) {
    float *pp = reinterpret_cast<float *>(&pv), *mm = reinterpret_cast<float *>(&mv), *vs = reinterpret_cast<float *>(&vv),
          *xx = reinterpret_cast<float *>(&xv);
    const float *gg = reinterpret_cast<const float *>(&gv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = wd != 0.f ? __fmaf_rn(wd, pp[e], gg[e]) : gg[e];         // grads + wd * params
        mm[e] = __fmaf_rn(one_m_b1, __fsub_rn(d, mm[e]), mm[e]);                 // exp_avg.lerp_(d, 1-b1) (small weight)
        vs[e] = __fmaf_rn(one_m_b2, __fmul_rn(d, d), __fmul_rn(b2, vs[e]));      // exp_avg_sq.mul_(b2).addcmul_(d, d, 1-b2)
        float s = vs[e];
        if (amsgrad) {
            xx[e] = (s != s || s > xx[e]) ? s : xx[e];                            // torch.maximum (NaN propagates)
            s = xx[e];
        }
        const float denom = __fadd_rn(sqrtf(s) / bc2_sqrt, eps);                 // sqrt(v) / bc2_sqrt + eps
        pp[e] = __fmaf_rn(step_size, mm[e] / denom, pp[e]);                       // params.addcdiv_(exp_avg, denom, step_size)
    }
}

__global__ void adam_flat_kernel(float4 *__restrict__ p, const float4 *__restrict__ g, float4 *__restrict__ m_,
                                 float4 *__restrict__ v_, float4 *__restrict__ vmax_, size_t n4, float one_m_b1, float b2,
                                 float one_m_b2, float eps, float wd, float step_size, float bc2_sqrt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 pv = p[i], mv = m_[i], vv = v_[i];
    const float4 gv = g[i];
    float4 xv = vmax_ ? vmax_[i] : make_float4(0, 0, 0, 0);
    adam_update4(pv, gv, mv, vv, xv, vmax_ != nullptr, one_m_b1, b2, one_m_b2, eps, wd, step_size, bc2_sqrt);
    p[i] = pv;
    m_[i] = mv;
    v_[i] = vv;
    if (vmax_) vmax_[i] = xv;
}

// ---- loss scaling (torch.amp.GradScaler's contract for optimisers with _step_supports_amp_scaling): no host read anywhere.
// found_inf / grad_scale / the applied-step count are device scalars; a launch whose found_inf != 0 writes nothing.

__device__ __forceinline__ unsigned nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// torch._amp_foreach_non_finite_check_and_unscale_ over the flat bucket: found_inf = 1 if any INPUT element is Inf / NaN
// (never reset: it accumulates like torch's), and g = inv == 1 ? g : g * inv when inv_scale is given (none: check only, the
// bucket is not written).  Grid-stride over float4; one plain store of 1.0f per wave that saw a non-finite value (every
// writer stores the same value).
__global__ void amp_check_unscale_flat_kernel(float4 *__restrict__ g, size_t n4, const float *__restrict__ inv_scale,
                                              float *__restrict__ found_inf) {
    const float inv = inv_scale ? *inv_scale : 1.f;
    const bool write = inv_scale != nullptr && inv != 1.f;
    unsigned bad = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 v = g[i];
        bad |= nonfinite(v.x) | nonfinite(v.y) | nonfinite(v.z) | nonfinite(v.w);
        if (write) g[i] = make_float4(__fmul_rn(v.x, inv), __fmul_rn(v.y, inv), __fmul_rn(v.z, inv), __fmul_rn(v.w, inv));
    }
    if (__any(bad != 0) && (threadIdx.x & 63) == 0) *found_inf = 1.f;
}

// GradScaler's unscale, as torch's unscale_ computes it: inv = (float)(1 / (double)scale), g = inv == 1 ? g : g * inv; the
// unscaled gradient is written back so the bucket holds what p.grad holds after a stock GradScaler step
__device__ __forceinline__ float4 amp_unscale4(float4 *__restrict__ g, size_t i, const float *__restrict__ grad_scale) {
    float4 gv = g[i];
    if (grad_scale) {
        const float inv = (float)(1.0 / (double)*grad_scale);
        if (inv != 1.f) {
            gv = make_float4(__fmul_rn(gv.x, inv), __fmul_rn(gv.y, inv), __fmul_rn(gv.z, inv), __fmul_rn(gv.w, inv));
            g[i] = gv;
        }
    }
    return gv;
}

// The applied-step counter advances in a separate one-thread launch on the same stream AFTER the update (stream order: no
// block of the update can still be reading it), and only when the step was applied.
__global__ void amp_count_applied_kernel(const float *__restrict__ found_inf, int64_t *__restrict__ applied) {
    if (*found_inf == 0.f) *applied += 1;
}

// Nesterov SGD with a device-side skip: "first step" (momentum buffer := d) is the first APPLIED step, applied == 0
__global__ void sgd_nesterov_flat_amp_kernel(float4 *__restrict__ p, float4 *__restrict__ g, float4 *__restrict__ buf, size_t n4,
                                             float lr, float mu, float damp, float wd, int nesterov,
                                             const float *__restrict__ grad_scale, const float *__restrict__ found_inf,
                                             const int64_t *__restrict__ applied) {
    if (*found_inf != 0.f) return;                                      // NaN counts as found, like GradScaler's sum != 0
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int first = *applied == 0;
    float4 pv = p[i];
    const float4 gv = amp_unscale4(g, i, grad_scale);
    float4 bv = (first || mu == 0.f) ? make_float4(0, 0, 0, 0) : buf[i];
    sgd_update4(pv, gv, bv, lr, mu, damp, wd, nesterov, first);
    p[i] = pv;
    if (mu != 0.f) buf[i] = bv;
}

// Adam with a device-side skip.  The step of this update is k = applied + 1; bias[2(k-1)], bias[2(k-1)+1] hold 1 - b1^k and
// sqrt(1 - b2^k) in double as the host computes them (cer_adam_flat / torch's Python floats).  Past the table's end the entries
// are constant (the host stops the table once both have reached 1.0), so the index is clamped.
__global__ void adam_flat_amp_kernel(float4 *__restrict__ p, float4 *__restrict__ g, float4 *__restrict__ m_, float4 *__restrict__ v_,
                                     float4 *__restrict__ vmax_, size_t n4, double lr, float one_m_b1, float b2, float one_m_b2,
                                     float eps, float wd, const double *__restrict__ bias, int64_t table_len,
                                     const float *__restrict__ grad_scale, const float *__restrict__ found_inf,
                                     const int64_t *__restrict__ applied) {
    if (*found_inf != 0.f) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int64_t k = *applied + 1;
    const int64_t j = (k < table_len ? k : table_len) - 1;
    const float step_size = (float)(lr / bias[2 * j] * -1.0);           // torch: (lr / bc) * -1 in double, then a float scalar
    const float bc2_sqrt = (float)bias[2 * j + 1];
    float4 pv = p[i], mv = m_[i], vv = v_[i];
    const float4 gv = amp_unscale4(g, i, grad_scale);
    float4 xv = vmax_ ? vmax_[i] : make_float4(0, 0, 0, 0);
    adam_update4(pv, gv, mv, vv, xv, vmax_ != nullptr, one_m_b1, b2, one_m_b2, eps, wd, step_size, bc2_sqrt);
    p[i] = pv;
    m_[i] = mv;
    v_[i] = vv;
    if (vmax_) vmax_[i] = xv;
}

__global__ void gather_rows_kernel(const float4 *__restrict__ src, const int64_t *__restrict__ index, float4 *__restrict__ out,
                                   int n_out, int cols4, int64_t n_src) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_out * cols4) return;
    const int r = (int)(i / cols4), c = (int)(i - (size_t)r * cols4);
    const int64_t s = index[r];
    out[i] = (s >= 0 && s < n_src) ? src[(size_t)s * cols4 + c] : make_float4(0, 0, 0, 0);
}

// channels-last PReLU with per-channel slopes (arcface_model.py:54): y = x > 0 ? x : alpha[c] * x
__global__ void prelu_fwd_kernel(const float4 *__restrict__ x, const float *__restrict__ alpha, float4 *__restrict__ y, size_t n4,
                                 int C4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 v = x[i], a = *reinterpret_cast<const float4 *>(alpha + (i % C4) * 4);
    y[i] = make_float4(v.x > 0.f ? v.x : a.x * v.x, v.y > 0.f ? v.y : a.y * v.y, v.z > 0.f ? v.z : a.z * v.z,
                       v.w > 0.f ? v.w : a.w * v.w);
}
// torch's prelu backward: dx = x > 0 ? dy : alpha[c]*dy; the slope gradient is the column sum of t = x > 0 ? 0 : x*dy
__global__ void prelu_bwd_kernel(const float4 *__restrict__ dy, const float4 *__restrict__ x, const float *__restrict__ alpha,
                                 float4 *__restrict__ dx, float4 *__restrict__ t, size_t n4, int C4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 g = dy[i], v = x[i], a = *reinterpret_cast<const float4 *>(alpha + (i % C4) * 4);
    dx[i] = make_float4(v.x > 0.f ? g.x : a.x * g.x, v.y > 0.f ? g.y : a.y * g.y, v.z > 0.f ? g.z : a.z * g.z,
                        v.w > 0.f ? g.w : a.w * g.w);
    t[i] = make_float4(v.x > 0.f ? 0.f : v.x * g.x, v.y > 0.f ? 0.f : v.y * g.y, v.z > 0.f ? 0.f : v.z * g.z,
                       v.w > 0.f ? 0.f : v.w * g.w);
}

// y = x / ||x||  ->  dx = (dy - y * (y . dy)) / ||x||   (one wave per row; reference models/arcface_model.py:17-20)
__global__ void l2norm_rows_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ x, float *__restrict__ dx,
                                       int rows, int cols) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float *xr = x + (size_t)row * cols, *gr = dy + (size_t)row * cols;
    float ss = 0.f, dot = 0.f;
    for (int c = lane; c < cols; c += 64) {
        ss += xr[c] * xr[c];
        dot += xr[c] * gr[c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_xor(ss, o);
        dot += __shfl_xor(dot, o);
    }
    const float inv = 1.f / sqrtf(ss);
    const float k = dot * inv * inv * inv;  // (y . dy) / ||x|| * (1/||x||) with y = x/||x||
    for (int c = lane; c < cols; c += 64) dx[(size_t)row * cols + c] = gr[c] * inv - xr[c] * k;
}

}  // namespace cer

using namespace cer;

extern "C" int cer_l2norm_rows_bwd(const float *dy, const float *x, float *dx, int rows, int cols, void *stream) {
    if (!dy || !x || !dx || rows <= 0 || cols <= 0) return cer_set_error(CER_ERR_INVALID_ARG, "l2norm_rows_bwd: bad argument");
    CER_LAUNCH(l2norm_rows_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, dy, x, dx, rows, cols);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_sgd_nesterov_flat(float *param, const float *grad, float *momentum_buf, size_t n, float lr, float momentum,
                                     float dampening, float weight_decay, int nesterov, int first_step, void *stream) {
    if (!param || !grad || n == 0 || (n & 3) || (momentum != 0.f && !momentum_buf))
        return cer_set_error(CER_ERR_INVALID_ARG, "sgd_nesterov_flat: needs param, grad, (momentum_buf), n a positive multiple of 4");
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf) & 15)
        return cer_set_error(CER_ERR_INVALID_ARG, "sgd_nesterov_flat: buffers must be 16-byte aligned");
    if (nesterov && (momentum <= 0.f || dampening != 0.f))
        return cer_set_error(CER_ERR_INVALID_ARG, "sgd_nesterov_flat: Nesterov momentum requires a momentum and zero dampening");
    CER_LAUNCH(sgd_nesterov_flat_kernel, dim3(cer_blocks(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, (float4 *)param,
               (const float4 *)grad, (float4 *)momentum_buf, n / 4, lr, momentum, dampening, weight_decay, nesterov, first_step);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_adam_flat(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq,
                             size_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int amsgrad,
                             int64_t step, void *stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n == 0 || (n & 3) || (amsgrad && !max_exp_avg_sq))
        return cer_set_error(CER_ERR_INVALID_ARG,
                             "adam_flat: needs param, grad, exp_avg, exp_avg_sq, (max_exp_avg_sq), n a positive multiple of 4");
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq |
         (uintptr_t)(amsgrad ? max_exp_avg_sq : nullptr)) & 15)
        return cer_set_error(CER_ERR_INVALID_ARG, "adam_flat: buffers must be 16-byte aligned");
    if (step < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return cer_set_error(CER_ERR_INVALID_ARG, "adam_flat: needs step >= 1 and betas in [0, 1)");
    // torch computes these in Python floats (double: `lr / bc * -1`, `bc ** 0.5`) and hands them to the foreach kernels as
    // float scalars
    const double step_size = lr / (1.0 - std::pow(beta1, (double)step)) * -1.0;
    const double bc2_sqrt = std::pow(1.0 - std::pow(beta2, (double)step), 0.5);
    CER_LAUNCH(adam_flat_kernel, dim3(cer_blocks(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, (float4 *)param,
               (const float4 *)grad, (float4 *)exp_avg, (float4 *)exp_avg_sq, amsgrad ? (float4 *)max_exp_avg_sq : nullptr, n / 4,
               (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)step_size,
               (float)bc2_sqrt);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_amp_check_unscale_flat(float *grad, size_t n, const float *inv_scale, float *found_inf, void *stream) {
    if (!grad || !found_inf || n == 0 || (n & 3))
        return cer_set_error(CER_ERR_INVALID_ARG, "amp_check_unscale_flat: needs grad, found_inf and n a positive multiple of 4");
    if (((uintptr_t)grad & 15) || (((uintptr_t)inv_scale | (uintptr_t)found_inf) & 3))
        return cer_set_error(CER_ERR_INVALID_ARG, "amp_check_unscale_flat: grad must be 16-byte aligned, the scalars 4-byte aligned");
    const unsigned blocks = cer_blocks(n / 4, 256) < 2048u ? cer_blocks(n / 4, 256) : 2048u;   // grid-stride beyond 2048 blocks
    CER_LAUNCH(amp_check_unscale_flat_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (float4 *)grad, n / 4, inv_scale,
               found_inf);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

static int amp_scalars_bad(const char *what, const float *grad_scale, const float *found_inf, const int64_t *applied) {
    if (!found_inf || !applied) return cer_set_error(CER_ERR_INVALID_ARG, "%s: needs found_inf and applied", what);
    if ((((uintptr_t)grad_scale | (uintptr_t)found_inf) & 3) || ((uintptr_t)applied & 7))
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: grad_scale / found_inf must be 4-byte aligned, applied 8-byte aligned", what);
    return CER_OK;
}

extern "C" int cer_sgd_nesterov_flat_amp(float *param, float *grad, float *momentum_buf, size_t n, float lr, float momentum,
                                         float dampening, float weight_decay, int nesterov, const float *grad_scale,
                                         const float *found_inf, int64_t *applied, void *stream) {
    if (!param || !grad || n == 0 || (n & 3) || (momentum != 0.f && !momentum_buf))
        return cer_set_error(CER_ERR_INVALID_ARG,
                             "sgd_nesterov_flat_amp: needs param, grad, (momentum_buf), n a positive multiple of 4");
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf) & 15)
        return cer_set_error(CER_ERR_INVALID_ARG, "sgd_nesterov_flat_amp: buffers must be 16-byte aligned");
    if (nesterov && (momentum <= 0.f || dampening != 0.f))
        return cer_set_error(CER_ERR_INVALID_ARG, "sgd_nesterov_flat_amp: Nesterov momentum requires a momentum and zero dampening");
    if (int rc = amp_scalars_bad("sgd_nesterov_flat_amp", grad_scale, found_inf, applied)) return rc;
    CER_LAUNCH(sgd_nesterov_flat_amp_kernel, dim3(cer_blocks(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, (float4 *)param,
               (float4 *)grad, (float4 *)momentum_buf, n / 4, lr, momentum, dampening, weight_decay, nesterov, grad_scale, found_inf,
               applied);
    CER_HIP_CHECK(hipGetLastError());
    CER_LAUNCH(amp_count_applied_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, found_inf, applied);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_adam_flat_amp(float *param, float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq, size_t n,
                                 double lr, double beta1, double beta2, double eps, double weight_decay, int amsgrad,
                                 const double *bias_correction, int64_t table_len, const float *grad_scale,
                                 const float *found_inf, int64_t *applied, void *stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n == 0 || (n & 3) || (amsgrad && !max_exp_avg_sq))
        return cer_set_error(CER_ERR_INVALID_ARG,
                             "adam_flat_amp: needs param, grad, exp_avg, exp_avg_sq, (max_exp_avg_sq), n a positive multiple of 4");
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq |
         (uintptr_t)(amsgrad ? max_exp_avg_sq : nullptr)) & 15)
        return cer_set_error(CER_ERR_INVALID_ARG, "adam_flat_amp: buffers must be 16-byte aligned");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return cer_set_error(CER_ERR_INVALID_ARG, "adam_flat_amp: needs betas in [0, 1)");
    if (!bias_correction || table_len < 1 || ((uintptr_t)bias_correction & 7))
        return cer_set_error(CER_ERR_INVALID_ARG, "adam_flat_amp: needs an 8-byte aligned bias-correction table of >= 1 entry");
    if (int rc = amp_scalars_bad("adam_flat_amp", grad_scale, found_inf, applied)) return rc;
    CER_LAUNCH(adam_flat_amp_kernel, dim3(cer_blocks(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, (float4 *)param,
               (float4 *)grad, (float4 *)exp_avg, (float4 *)exp_avg_sq, amsgrad ? (float4 *)max_exp_avg_sq : nullptr, n / 4, lr,
               (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, bias_correction,
               table_len, grad_scale, found_inf, applied);
    CER_HIP_CHECK(hipGetLastError());
    CER_LAUNCH(amp_count_applied_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, found_inf, applied);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_gather_rows(const float *src, const int64_t *index, float *out, int n_out, int cols, int64_t n_src,
                               void *stream) {
    if (!src || !index || !out || n_out <= 0 || cols <= 0 || (cols & 3) || n_src <= 0)
        return cer_set_error(CER_ERR_INVALID_ARG, "gather_rows: needs src, index, out and cols % 4 == 0");
    CER_LAUNCH(gather_rows_kernel, dim3(cer_blocks((size_t)n_out * (cols / 4), 256)), dim3(256), 0, (hipStream_t)stream,
               (const float4 *)src, index, (float4 *)out, n_out, cols / 4, n_src);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_prelu_fwd(const float *x, const float *alpha, float *y, size_t rows, int C, void *stream) {
    if (!x || !alpha || !y || rows == 0 || C <= 0 || (C & 3)) return cer_set_error(CER_ERR_INVALID_ARG, "prelu_fwd: C % 4 == 0");
    const size_t n4 = rows * (C / 4);
    CER_LAUNCH(prelu_fwd_kernel, dim3(cer_blocks(n4, 256)), dim3(256), 0, (hipStream_t)stream, (const float4 *)x, alpha, (float4 *)y,
               n4, C / 4);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_prelu_bwd(const float *dy, const float *x, const float *alpha, float *dx, float *dalpha_terms, size_t rows,
                             int C, void *stream) {
    if (!dy || !x || !alpha || !dx || !dalpha_terms || rows == 0 || C <= 0 || (C & 3))
        return cer_set_error(CER_ERR_INVALID_ARG, "prelu_bwd: C % 4 == 0");
    const size_t n4 = rows * (C / 4);
    CER_LAUNCH(prelu_bwd_kernel, dim3(cer_blocks(n4, 256)), dim3(256), 0, (hipStream_t)stream, (const float4 *)dy, (const float4 *)x,
               alpha, (float4 *)dx, (float4 *)dalpha_terms, n4, C / 4);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}
