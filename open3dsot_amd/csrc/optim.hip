// optim.hip -- the rest of the flat-buffer optimizer family next to o3d_adam_step (csrc/heads.hip): the total gradient
// norm with torch.nn.utils.clip_grad_norm_'s coefficient, Adam on scaled gradients, and torch.optim.SGD with momentum
// (models/base_model.py:29-31; main.py:85 `gradient_clip_val`).  All three walk o3d_adam_step's DEVICE job table of
// njobs x 3 longs {gradient pointer, offset of the parameter in the flat buffers, element count}; block (job, slice) takes
// elements slice*256 + thread, + 256 * slices, ... of its job, so a gradient on any 4-byte boundary is read coalesced.
//
// Built with -ffp-contract=off: the operation order written here IS the contract (tests/optim_oracle.py restates it).
#include "o3d_common.hpp"

namespace {

// sum over the 256 threads of a block, valid in thread 0: a butterfly over each wave's 64 lanes (32, 16, ..., 1), then the
// four wave sums through LDS as (w0 + w1) + (w2 + w3).  The order is fixed: the same inputs give the same bits.
__device__ __forceinline__ double block_sum_256(double s, double* sh) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// launch 1 of o3d_grad_norm: partials[job * slices + slice] = sum of g^2 over the slice's elements, in double.  Every block
// stores, so `partials` needs no clearing; a slice that holds no element stores 0.
__global__ __launch_bounds__(256) void grad_sqsum_kernel(const long* __restrict__ jobs, double* __restrict__ partials) {
    __shared__ double sh[4];
    const long* j = jobs + 3L * blockIdx.x;
    const float* g = reinterpret_cast<const float*>(j[0]);
    const long n = j[2];
    double s = 0.0;
    for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < n; i += 256L * gridDim.y) {
        const double gi = (double)g[i];
        s += gi * gi;
    }
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) partials[(long)blockIdx.x * gridDim.y + blockIdx.y] = s;
}

// launch 2: one block adds the partials -- thread t takes t, t + 256, ... in that order, then block_sum_256 -- and writes
// the norm and clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)), both rounded to float once.  `c > 1 ? 1 : c`
// keeps a NaN coefficient a NaN, as torch.clamp(max=1) does.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partials, int count,
                                                               double max_norm, float* __restrict__ out) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) s += partials[i];
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) {
        const double nrm = sqrt(s);
        const double c = max_norm / (nrm + 1e-6);
        out[0] = (float)nrm;
        out[1] = (float)(c > 1.0 ? 1.0 : c);
    }
}

// adam_step_kernel of csrc/heads.hip on g * *grad_scale, the body repeated.  That file is built with the compiler's default
// contraction, but its code for this body holds no fused operation beyond the written fmaf's (`sqrtf(v) * inv_sqrt_bc2 + eps`
// is a multiply and an add there: the multiply is packed with lr_bc1 * m), so the same expressions without contraction give
// the same bits; tests/test_optim_kernels_gpu.py holds the two kernels together at scales 1 and 0.5.
__global__ __launch_bounds__(256) void adam_step_scaled_kernel(const long* __restrict__ jobs, float* __restrict__ P,
                                                               float* __restrict__ M, float* __restrict__ V, float lr_bc1,
                                                               float beta1, float omb1, float beta2, float omb2, float eps,
                                                               float wd, float inv_sqrt_bc2,
                                                               const float* __restrict__ grad_scale) {
    const long* j = jobs + 3L * blockIdx.x;
    const float* g = reinterpret_cast<const float*>(j[0]);
    const long off = j[1], n = j[2];
    const float scale = *grad_scale;
    for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < n; i += 256L * gridDim.y) {
        const long k = off + i;
        float p = P[k];
        float gi = g[i] * scale;
        if (wd != 0.f) gi = fmaf(wd, p, gi);
        const float m = fmaf(beta1, M[k], omb1 * gi);
        const float v = fmaf(beta2, V[k], omb2 * gi * gi);
        M[k] = m; V[k] = v;
        P[k] = p - lr_bc1 * m / (sqrtf(v) * inv_sqrt_bc2 + eps);
    }
}

// torch.optim.SGD with momentum, dampening 0, no Nesterov.  A zero buffer gives buf = g' exactly (fma(momentum, 0, g')),
// which is torch's first-step rule: no "first step" flag.
__global__ __launch_bounds__(256) void sgd_step_kernel(const long* __restrict__ jobs, float* __restrict__ P,
                                                       float* __restrict__ B, float neg_lr, float momentum, float wd,
                                                       const float* __restrict__ grad_scale) {
    const long* j = jobs + 3L * blockIdx.x;
    const float* g = reinterpret_cast<const float*>(j[0]);
    const long off = j[1], n = j[2];
    const bool scaled = grad_scale != nullptr;
    const float scale = scaled ? *grad_scale : 1.f;
    for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < n; i += 256L * gridDim.y) {
        const long k = off + i;
        const float p = P[k];
        float gi = g[i];
        if (scaled) gi = gi * scale;
        if (wd != 0.f) gi = fmaf(wd, p, gi);
        const float b = fmaf(momentum, B[k], gi);
        B[k] = b;
        P[k] = fmaf(neg_lr, b, p);
    }
}

}  // namespace

// Total 2-norm of the gradients of a job table and the clipping coefficient, two plain launches in stream order (no
// atomics, no tickets): partials (njobs * O3D_NORM_SLICES doubles, every one written), out[0] = (float)sqrt(S),
// out[1] = (float)min(1, max_norm / (sqrt(S) + 1e-6)).  Non-finite gradients follow the arithmetic (out[0] shows them).
extern "C" int o3d_grad_norm(const long* jobs, int njobs, double max_norm, double* partials, float* out, void* stream) {
    if (!jobs || njobs <= 0 || !partials || !out || !(max_norm > 0.)) return O3D_EINVAL;
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3(njobs, O3D_NORM_SLICES), dim3(256), 0, o3d_stream(stream), jobs, partials);
    if (o3d_launch_status() != O3D_OK) return O3D_ELAUNCH;
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, o3d_stream(stream), partials,
                       njobs * O3D_NORM_SLICES, max_norm, out);
    return o3d_launch_status();
}

// o3d_adam_step with every gradient multiplied by *grad_scale (a DEVICE float, e.g. out + 1 of o3d_grad_norm) before the
// weight decay: clipping precedes the optimizer.
extern "C" int o3d_adam_step_scaled(const long* jobs, int njobs, float* params, float* exp_avg, float* exp_avg_sq,
                                    double lr, double beta1, double beta2, double eps, double weight_decay, double bc1,
                                    double bc2, const float* grad_scale, void* stream) {
    if (!jobs || njobs <= 0 || !params || !exp_avg || !exp_avg_sq || !grad_scale || bc1 <= 0. || bc2 <= 0.) return O3D_EINVAL;
    hipLaunchKernelGGL(adam_step_scaled_kernel, dim3(njobs, 32), dim3(256), 0, o3d_stream(stream), jobs, params, exp_avg,
                       exp_avg_sq, (float)(lr / bc1), (float)beta1, (float)(1. - beta1), (float)beta2, (float)(1. - beta2),
                       (float)eps, (float)weight_decay, (float)(1.0 / sqrt(bc2)), grad_scale);
    return o3d_launch_status();
}

// One SGD step on the flat buffers, in this order per element (each line one rounding):
//   g' = g * *grad_scale          when grad_scale is given (NULL: g' = g)
//   g' = fma(weight_decay, p, g')  when weight_decay != 0
//   buf = fma(momentum, buf, g')
//   p = fma(-lr, buf, p)
extern "C" int o3d_sgd_step(const long* jobs, int njobs, float* params, float* momentum_buf, double lr, double momentum,
                            double weight_decay, const float* grad_scale, void* stream) {
    if (!jobs || njobs <= 0 || !params || !momentum_buf || !(lr >= 0.) || !(momentum >= 0.) || !(weight_decay >= 0.))
        return O3D_EINVAL;
    hipLaunchKernelGGL(sgd_step_kernel, dim3(njobs, 32), dim3(256), 0, o3d_stream(stream), jobs, params, momentum_buf,
                       -(float)lr, (float)momentum, (float)weight_decay, grad_scale);
    return o3d_launch_status();
}
