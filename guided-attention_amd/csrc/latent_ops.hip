// K5/K6 and the CFG+DDIM step: element-wise latent updates (16 384 elements for SD-1.x 512^2).
//   ga_latent_axpy  : out = latents - step*grad (+ fused mean|grad|)   pipeline_guided_attention.py:466-469
//   ga_latent_axpby : out = a*x + b*y (re-noise)                       pipeline_guided_attention.py:1048-1053
//   ga_cfg_ddim_step: CFG combine + DDIM eta=0 update                  pipeline_guided_attention.py:1022-1029
//   ga_cfg_ddim_step_pred: the same step for a UNet that predicts v or the sample (the scheduler's prediction_type)
//   ga_cfg_ddim_step_eta: the step with eta > 0 (stochastic DDIM): the caller's variance noise is one more operand
//   ga_latent_sgd_momentum: b = mu*b + g, out = latents - lr*b (use_optimizer) pipeline_guided_attention.py:497,549-551
// Launch-latency bound; one pass, math in f32, one rounding to T at the store.
// Batched forms (S images of n elements each, image-major): per-image `active` flags / steps in device memory (captured
// graphs read them from static buffers); an inactive image is copied through bit for bit, an active one gets exactly the
// element formula (and, for the axpy, the reduction order) of the single-image launch on its slice.
//   ga_latent_sgd_momentum_batched: the momentum step per image, with per-image lr / first / active in device memory.
#include "ga_common.h"

using namespace ga;

namespace {

template <typename T>
__global__ __launch_bounds__(256) void axpby_kernel(const T* __restrict__ x, const T* __restrict__ y, float a, float b,
                                                    T* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    out[i] = Traits<T>::from_f32(a * Traits<T>::to_f32(x[i]) + b * Traits<T>::to_f32(y[i]));
}

template <typename T>
__device__ __forceinline__ T axpy_elem(T x, float step, float g) {
  return Traits<T>::from_f32(Traits<T>::to_f32(x) - step * g);
}

template <typename T>
__global__ __launch_bounds__(256) void axpy_kernel(const T* __restrict__ x, const T* __restrict__ g, float step,
                                                   T* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    out[i] = axpy_elem<T>(x[i], step, Traits<T>::to_f32(g[i]));
}

// single workgroup: also reduces sum|grad| deterministically (same element formula as axpy_kernel)
template <typename T>
__global__ __launch_bounds__(1024) void axpy_absmean_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                            float step, T* __restrict__ out,
                                                            float* __restrict__ absmean, long long n) {
  __shared__ float part[16];
  float acc = 0.f;
  for (long long i = threadIdx.x; i < n; i += 1024) {
    const float gv = Traits<T>::to_f32(g[i]);
    acc += fabsf(gv);
    out[i] = axpy_elem<T>(x[i], step, gv);
  }
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < 16; ++w) s += part[w];
    absmean[0] = s / (float)n;
  }
}

// The DDIM step for a model output that is not the noise (GA_PRED_V, GA_PRED_SAMPLE): the CFG combine m = u + gs * (t - u), then
//   v:      x0 = sa_t * x - s1_t * m,  eps = sa_t * m + s1_t * x          sample:  x0 = m,  eps = (x - sa_t * m) / s1_t
// and prev = sa_p * x0 + s1_p * eps.  ONE element function for the single-image and the masked kernel, every multiply-add an
// explicit fma and every f32 result fenced in front of its rounding to T (sgd_elem tells why), so an active image of the
// masked launch has the bits of the single-image launch on its slice.  GA_PRED_EPSILON is not served here: its expressions
// stand in the two kernels as they always have.
template <typename T>
__device__ __forceinline__ T round_to(float r) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(r));
#endif
  return Traits<T>::from_f32(r);
}
template <typename T, int PRED>
__device__ __forceinline__ void ddim_pred_elem(T uv, T tv, T xv, float gs, float sa_t, float s1_t, float sa_p, float s1_p,
                                               T& prev, T& x0o) {
  static_assert(PRED == GA_PRED_V || PRED == GA_PRED_SAMPLE, "the epsilon form keeps its own expressions");
  const float u = Traits<T>::to_f32(uv), x = Traits<T>::to_f32(xv);
  const float m = __builtin_fmaf(gs, Traits<T>::to_f32(tv) - u, u);
  float x0, eps;
  if constexpr (PRED == GA_PRED_V) {
    x0 = __builtin_fmaf(sa_t, x, -(s1_t * m));
    eps = __builtin_fmaf(sa_t, m, s1_t * x);
  } else {
    x0 = m;
    eps = __builtin_fmaf(-sa_t, m, x) / s1_t;
  }
  x0o = round_to<T>(x0);
  prev = round_to<T>(__builtin_fmaf(sa_p, x0, s1_p * eps));
}

template <typename T, int PRED>
__global__ __launch_bounds__(256) void cfg_ddim_kernel(const T* __restrict__ eu, const T* __restrict__ et, float gs,
                                                       const T* __restrict__ x, float sa_t, float s1_t, float sa_p,
                                                       float s1_p, T* __restrict__ prev, T* __restrict__ x0o,
                                                       long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    if constexpr (PRED == GA_PRED_EPSILON) {
      const float u = Traits<T>::to_f32(eu[i]);
      const float eps = u + gs * (Traits<T>::to_f32(et[i]) - u);
      const float x0 = (Traits<T>::to_f32(x[i]) - s1_t * eps) / sa_t;
      if (x0o) x0o[i] = Traits<T>::from_f32(x0);
      prev[i] = Traits<T>::from_f32(sa_p * x0 + s1_p * eps);
    } else {
      T pv, x0v;
      ddim_pred_elem<T, PRED>(eu[i], et[i], x[i], gs, sa_t, s1_t, sa_p, s1_p, pv, x0v);
      if (x0o) x0o[i] = x0v;
      prev[i] = pv;
    }
  }
}

// one 1024-thread workgroup per image (blockIdx.x): axpy_absmean_kernel's loop and reduction on that image's slice
template <typename T>
__global__ __launch_bounds__(1024) void axpy_batched_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                            const float* __restrict__ step, const int* __restrict__ active,
                                                            T* __restrict__ out, float* __restrict__ absmean, long long n) {
  __shared__ float part[16];
  const size_t off = (size_t)blockIdx.x * n;
  x += off;
  g += off;
  out += off;
  const int on = active[blockIdx.x];
  const float st = step[blockIdx.x];
  if (!on) {
    for (long long i = threadIdx.x; i < n; i += 1024) out[i] = x[i];
    return;
  }
  float acc = 0.f;
  for (long long i = threadIdx.x; i < n; i += 1024) {
    const float gv = Traits<T>::to_f32(g[i]);
    acc += fabsf(gv);
    out[i] = axpy_elem<T>(x[i], st, gv);
  }
  if (!absmean) return;
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < 16; ++w) s += part[w];
    absmean[blockIdx.x] = s / (float)n;
  }
}

// masked forms over all S * n elements: the flag is loaded with the operands (no load waits on another) and selects at the store
template <typename T>
__global__ __launch_bounds__(256) void axpby_masked_kernel(const T* __restrict__ x, const T* __restrict__ y, float a, float b,
                                                           const int* __restrict__ active, T* __restrict__ out, long long n,
                                                           long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const T xv = x[i], yv = y[i];
    const int on = active[i / n];
    out[i] = on ? Traits<T>::from_f32(a * Traits<T>::to_f32(xv) + b * Traits<T>::to_f32(yv)) : xv;
  }
}

template <typename T, int PRED>
__global__ __launch_bounds__(256) void cfg_ddim_masked_kernel(const T* __restrict__ eu, const T* __restrict__ et, float gs,
                                                              const T* __restrict__ x, float sa_t, float s1_t, float sa_p,
                                                              float s1_p, const int* __restrict__ active, T* __restrict__ prev,
                                                              T* __restrict__ x0o, long long n, long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const T uv = eu[i], tv = et[i], xv = x[i];
    const int on = active[i / n];
    if constexpr (PRED == GA_PRED_EPSILON) {
      const float u = Traits<T>::to_f32(uv);
      const float eps = u + gs * (Traits<T>::to_f32(tv) - u);
      const float x0 = (Traits<T>::to_f32(xv) - s1_t * eps) / sa_t;
      if (x0o) x0o[i] = Traits<T>::from_f32(x0);   // inactive images too: no element of x0_out is left unwritten
      prev[i] = on ? Traits<T>::from_f32(sa_p * x0 + s1_p * eps) : xv;
    } else {
      T pv, x0v;
      ddim_pred_elem<T, PRED>(uv, tv, xv, gs, sa_t, s1_t, sa_p, s1_p, pv, x0v);
      if (x0o) x0o[i] = x0v;   // inactive images too
      prev[i] = on ? pv : xv;
    }
  }
}

// The stochastic DDIM step (0 < eta <= 1, Song et al. eq. 12 / 16) for all three prediction types: m, x0 and eps by the table of
// ga_hip.h, then prev = sa_p * x0 + c_dir * eps + sigma * z with z the caller's variance noise; the host hands over
// sigma = eta * sqrt(var) and c_dir = sqrt(1 - a_p - sigma^2).  ONE element function for the single-image and the masked kernel,
// in ddim_pred_elem's style (explicit fmas, every f32 result fenced in front of its rounding to T), so an active image of the
// masked launch has the bits of the single-image launch on its slice.  z enters prev only: x0 does not depend on it.
template <typename T, int PRED>
__device__ __forceinline__ void ddim_eta_elem(T uv, T tv, T xv, T zv, float gs, float sa_t, float s1_t, float sa_p, float c_dir,
                                              float sigma, T& prev, T& x0o) {
  const float u = Traits<T>::to_f32(uv), x = Traits<T>::to_f32(xv);
  const float m = __builtin_fmaf(gs, Traits<T>::to_f32(tv) - u, u);
  float x0, eps;
  if constexpr (PRED == GA_PRED_EPSILON) {
    x0 = __builtin_fmaf(-s1_t, m, x) / sa_t;
    eps = m;
  } else if constexpr (PRED == GA_PRED_V) {
    x0 = __builtin_fmaf(sa_t, x, -(s1_t * m));
    eps = __builtin_fmaf(sa_t, m, s1_t * x);
  } else {
    static_assert(PRED == GA_PRED_SAMPLE, "one of the three GA_PRED_* values");
    x0 = m;
    eps = __builtin_fmaf(-sa_t, m, x) / s1_t;
  }
  x0o = round_to<T>(x0);
  prev = round_to<T>(__builtin_fmaf(sa_p, x0, __builtin_fmaf(c_dir, eps, sigma * Traits<T>::to_f32(zv))));
}

template <typename T, int PRED>
__global__ __launch_bounds__(256) void cfg_ddim_eta_kernel(const T* __restrict__ eu, const T* __restrict__ et, float gs,
                                                           const T* __restrict__ x, const T* __restrict__ z, float sa_t,
                                                           float s1_t, float sa_p, float c_dir, float sigma,
                                                           T* __restrict__ prev, T* __restrict__ x0o, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    T pv, x0v;
    ddim_eta_elem<T, PRED>(eu[i], et[i], x[i], z[i], gs, sa_t, s1_t, sa_p, c_dir, sigma, pv, x0v);
    if (x0o) x0o[i] = x0v;
    prev[i] = pv;
  }
}

// the masked form over all S * n elements: the noise of an inactive image is loaded with the other operands and dropped with pv
// by the select at the store (it may hold NaN patterns: never multiplied into what is stored)
template <typename T, int PRED>
__global__ __launch_bounds__(256) void cfg_ddim_eta_masked_kernel(const T* __restrict__ eu, const T* __restrict__ et, float gs,
                                                                  const T* __restrict__ x, const T* __restrict__ z, float sa_t,
                                                                  float s1_t, float sa_p, float c_dir, float sigma,
                                                                  const int* __restrict__ active, T* __restrict__ prev,
                                                                  T* __restrict__ x0o, long long n, long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const T uv = eu[i], tv = et[i], xv = x[i], zv = z[i];
    const int on = active[i / n];
    T pv, x0v;
    ddim_eta_elem<T, PRED>(uv, tv, xv, zv, gs, sa_t, s1_t, sa_p, c_dir, sigma, pv, x0v);
    if (x0o) x0o[i] = x0v;   // inactive images too
    prev[i] = on ? pv : xv;
  }
}

int grid_for(long long n) { return (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048); }

// The launch behind ga_cfg_ddim_step[_masked] (PRED = GA_PRED_EPSILON) and ga_cfg_ddim_step_pred[_masked]: epsilon is one
// instantiation whichever entry asks for it.  active == NULL: the single-image kernel over n elements.
template <typename T, int PRED>
void launch_cfg_ddim(const void* eu, const void* et, float gs, const void* x, float alpha_t, float alpha_prev, const int* active,
                     void* prev, void* x0o, int images, long long n, hipStream_t s) {
  const float sa_t = sqrtf(alpha_t), s1_t = sqrtf(1.0f - alpha_t), sa_p = sqrtf(alpha_prev), s1_p = sqrtf(1.0f - alpha_prev);
  if (!active) {
    hipLaunchKernelGGL((cfg_ddim_kernel<T, PRED>), dim3(grid_for(n)), dim3(256), 0, s, (const T*)eu, (const T*)et, gs,
                       (const T*)x, sa_t, s1_t, sa_p, s1_p, (T*)prev, (T*)x0o, n);
  } else {
    const long long total = (long long)images * n;
    hipLaunchKernelGGL((cfg_ddim_masked_kernel<T, PRED>), dim3(grid_for(total)), dim3(256), 0, s, (const T*)eu, (const T*)et,
                       gs, (const T*)x, sa_t, s1_t, sa_p, s1_p, active, (T*)prev, (T*)x0o, n, total);
  }
}

template <typename T>
int do_cfg_ddim(int pred, const void* eu, const void* et, float gs, const void* x, float alpha_t, float alpha_prev,
                const int* active, void* prev, void* x0o, int images, long long n, hipStream_t s) {
  if (pred == GA_PRED_V)
    launch_cfg_ddim<T, GA_PRED_V>(eu, et, gs, x, alpha_t, alpha_prev, active, prev, x0o, images, n, s);
  else if (pred == GA_PRED_SAMPLE)
    launch_cfg_ddim<T, GA_PRED_SAMPLE>(eu, et, gs, x, alpha_t, alpha_prev, active, prev, x0o, images, n, s);
  else
    launch_cfg_ddim<T, GA_PRED_EPSILON>(eu, et, gs, x, alpha_t, alpha_prev, active, prev, x0o, images, n, s);
  return check_launch();
}

// host-side checks shared by the four cfg_ddim entries (before any launch): sizes, alphas in (0, 1] (a NaN fails every
// comparison), the prediction type, and no division by sqrt(1 - alpha_t) = 0 for a sample prediction
int cfg_ddim_args_ok(long long n, int images, float alpha_t, float alpha_prev, int pred) {
  if (n < 1 || images < 1 || images > GA_MAX_IMAGES) return 0;
  if (!(alpha_t > 0.f) || !(alpha_prev > 0.f) || !(alpha_t <= 1.f) || !(alpha_prev <= 1.f)) return 0;
  if (pred != GA_PRED_EPSILON && pred != GA_PRED_V && pred != GA_PRED_SAMPLE) return 0;
  if (pred == GA_PRED_SAMPLE && !(alpha_t < 1.f)) return 0;
  return 1;
}

int cfg_ddim_entry(int pred, const void* eu, const void* et, float gs, const void* x, float alpha_t, float alpha_prev,
                   const int* active, void* prev, void* x0o, int images, int64_t n, int dtype, ga_stream_t stream) {
  if (!cfg_ddim_args_ok(n, images, alpha_t, alpha_prev, pred)) return GA_ERR_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case GA_F16:
      return do_cfg_ddim<_Float16>(pred, eu, et, gs, x, alpha_t, alpha_prev, active, prev, x0o, images, n, s);
    case GA_BF16:
      return do_cfg_ddim<bf16_t>(pred, eu, et, gs, x, alpha_t, alpha_prev, active, prev, x0o, images, n, s);
    case GA_F32:
      return do_cfg_ddim<float>(pred, eu, et, gs, x, alpha_t, alpha_prev, active, prev, x0o, images, n, s);
    default:
      return GA_ERR_DTYPE;
  }
}

// The launches behind ga_cfg_ddim_step_eta[_masked] for eta > 0.  Coefficients in double from the arguments as received, each
// rounded once to f32.  active == NULL: the single-image kernel over n elements.
struct EtaCoef {
  float sa_t, s1_t, sa_p, c_dir, sigma;
};

EtaCoef eta_coefficients(float alpha_t, float alpha_prev, float eta) {
  const double a_t = alpha_t, a_p = alpha_prev;
  const double var = (1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p);
  const double sigma = (double)eta * sqrt(var > 0.0 ? var : 0.0);
  const double dir2 = 1.0 - a_p - sigma * sigma;
  return {(float)sqrt(a_t), (float)sqrt(1.0 - a_t), (float)sqrt(a_p), (float)sqrt(dir2 > 0.0 ? dir2 : 0.0), (float)sigma};
}

template <typename T, int PRED>
void launch_cfg_ddim_eta(const void* eu, const void* et, float gs, const void* x, const void* z, const EtaCoef& c,
                         const int* active, void* prev, void* x0o, int images, long long n, hipStream_t s) {
  if (!active) {
    hipLaunchKernelGGL((cfg_ddim_eta_kernel<T, PRED>), dim3(grid_for(n)), dim3(256), 0, s, (const T*)eu, (const T*)et, gs,
                       (const T*)x, (const T*)z, c.sa_t, c.s1_t, c.sa_p, c.c_dir, c.sigma, (T*)prev, (T*)x0o, n);
  } else {
    const long long total = (long long)images * n;
    hipLaunchKernelGGL((cfg_ddim_eta_masked_kernel<T, PRED>), dim3(grid_for(total)), dim3(256), 0, s, (const T*)eu,
                       (const T*)et, gs, (const T*)x, (const T*)z, c.sa_t, c.s1_t, c.sa_p, c.c_dir, c.sigma, active, (T*)prev,
                       (T*)x0o, n, total);
  }
}

template <typename T>
int do_cfg_ddim_eta(int pred, const void* eu, const void* et, float gs, const void* x, const void* z, const EtaCoef& c,
                    const int* active, void* prev, void* x0o, int images, long long n, hipStream_t s) {
  if (pred == GA_PRED_V)
    launch_cfg_ddim_eta<T, GA_PRED_V>(eu, et, gs, x, z, c, active, prev, x0o, images, n, s);
  else if (pred == GA_PRED_SAMPLE)
    launch_cfg_ddim_eta<T, GA_PRED_SAMPLE>(eu, et, gs, x, z, c, active, prev, x0o, images, n, s);
  else
    launch_cfg_ddim_eta<T, GA_PRED_EPSILON>(eu, et, gs, x, z, c, active, prev, x0o, images, n, s);
  return check_launch();
}

// eta == 0 is the launch of ga_cfg_ddim_step_pred[_masked] (the noise is not read); what eta > 0 adds to the host-side checks:
// eta in [0, 1] (a NaN fails the comparison), no division by 1 - alpha_t = 0, and alpha_t <= alpha_prev (the variance is >= 0)
int cfg_ddim_eta_entry(int pred, const void* eu, const void* et, float gs, const void* x, const void* z, float alpha_t,
                       float alpha_prev, float eta, const int* active, void* prev, void* x0o, int images, int64_t n, int dtype,
                       ga_stream_t stream) {
  if (!cfg_ddim_args_ok(n, images, alpha_t, alpha_prev, pred)) return GA_ERR_SHAPE;
  if (!(eta >= 0.f && eta <= 1.f)) return GA_ERR_SHAPE;
  if (eta == 0.f) return cfg_ddim_entry(pred, eu, et, gs, x, alpha_t, alpha_prev, active, prev, x0o, images, n, dtype, stream);
  if (!(alpha_t < 1.f) || alpha_t > alpha_prev) return GA_ERR_SHAPE;
  const EtaCoef c = eta_coefficients(alpha_t, alpha_prev, eta);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case GA_F16:
      return do_cfg_ddim_eta<_Float16>(pred, eu, et, gs, x, z, c, active, prev, x0o, images, n, s);
    case GA_BF16:
      return do_cfg_ddim_eta<bf16_t>(pred, eu, et, gs, x, z, c, active, prev, x0o, images, n, s);
    case GA_F32:
      return do_cfg_ddim_eta<float>(pred, eu, et, gs, x, z, c, active, prev, x0o, images, n, s);
    default:
      return GA_ERR_DTYPE;
  }
}

// SGD with momentum (torch.optim.SGD, dampening 0, no Nesterov): b = FIRST ? g : mu * b_old + g, x <- x - lr * b.  Both
// multiply-adds are explicit fmas, so the 16-byte and the element-wise path give the same bits for the same values.
__device__ __forceinline__ float sgd_velocity(float mu, float b_old, float g) { return __builtin_fmaf(mu, b_old, g); }
template <typename T>
__device__ __forceinline__ T sgd_elem(T x, float lr, float b) {
  float r = __builtin_fmaf(-lr, b, Traits<T>::to_f32(x));
#if defined(__HIP_DEVICE_COMPILE__)
  // The f32 result exists as such before it is rounded to T.  Without this the compiler folds fma + conversion of the
  // element-wise f16 path into v_fma_mixlo_f16, which rounds the exact sum to f16 ONCE, while the 16-byte path rounds to f32
  // and then to f16 (v_pk_fma_f32 + v_cvt_pk_f16_f32): the two paths then differ in the last bit of a few elements (seen on
  // the MI355X with `[1:]` slices against aligned copies of the same values).
  asm("" : "+v"(r));
#endif
  return Traits<T>::from_f32(r);
}

// 16 bytes of T as one vector register group: 4 f32, or 8 16-bit patterns
template <typename T>
struct Pack {
  typedef short vec __attribute__((ext_vector_type(8)));
  static constexpr int N = 8;
  __device__ static __forceinline__ T get(const vec& v, int i) { return __builtin_bit_cast(T, (short)v[i]); }
  __device__ static __forceinline__ void set(vec& v, int i, T e) { v[i] = __builtin_bit_cast(short, e); }
};
template <>
struct Pack<float> {
  typedef f32x4 vec;
  static constexpr int N = 4;
  __device__ static __forceinline__ float get(const vec& v, int i) { return v[i]; }
  __device__ static __forceinline__ void set(vec& v, int i, float e) { v[i] = e; }
};

// FIRST: the velocity buffer is written and never read.  VEC (every pointer 16-byte aligned): n / N whole vectors per grid-stride
// step, the n % N elements behind them one by one; otherwise every element one by one.  x and out may be the same tensor.
template <typename T, bool FIRST, bool VEC>
__global__ __launch_bounds__(256) void sgd_momentum_kernel(const T* x, const T* __restrict__ g, float* __restrict__ m, float lr,
                                                           float mu, T* out, long long n) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  long long done = 0;
  if constexpr (VEC) {
    using P = Pack<T>;
    constexpr int N = P::N;
    const long long nv = n / N;
    for (long long v = tid; v < nv; v += stride) {
      const typename P::vec xv = reinterpret_cast<const typename P::vec*>(x)[v];
      const typename P::vec gv = reinterpret_cast<const typename P::vec*>(g)[v];
      f32x4* mv = reinterpret_cast<f32x4*>(m) + v * (N / 4);
      f32x4 b[N / 4];
      if constexpr (!FIRST) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) b[q] = mv[q];
      }
      typename P::vec ov;
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float ge = Traits<T>::to_f32(P::get(gv, e));
        const float be = FIRST ? ge : sgd_velocity(mu, b[e / 4][e % 4], ge);
        b[e / 4][e % 4] = be;
        P::set(ov, e, sgd_elem<T>(P::get(xv, e), lr, be));
      }
#pragma unroll
      for (int q = 0; q < N / 4; ++q) mv[q] = b[q];
      reinterpret_cast<typename P::vec*>(out)[v] = ov;
    }
    done = nv * N;
  }
  for (long long i = done + tid; i < n; i += stride) {
    const float ge = Traits<T>::to_f32(g[i]);
    const float be = FIRST ? ge : sgd_velocity(mu, m[i], ge);
    const T xe = x[i];
    m[i] = be;
    out[i] = sgd_elem<T>(xe, lr, be);
  }
}

template <typename T>
int do_sgd_momentum(const void* x, const void* g, float* m, float lr, float mu, int first, void* out, long long n, hipStream_t s) {
  const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                     reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const dim3 grid(grid_for(vec ? (n + Pack<T>::N - 1) / Pack<T>::N : n)), block(256);
  const T *xp = (const T*)x, *gp = (const T*)g;
  T* op = (T*)out;
  if (first && vec)
    hipLaunchKernelGGL((sgd_momentum_kernel<T, true, true>), grid, block, 0, s, xp, gp, m, lr, mu, op, n);
  else if (first)
    hipLaunchKernelGGL((sgd_momentum_kernel<T, true, false>), grid, block, 0, s, xp, gp, m, lr, mu, op, n);
  else if (vec)
    hipLaunchKernelGGL((sgd_momentum_kernel<T, false, true>), grid, block, 0, s, xp, gp, m, lr, mu, op, n);
  else
    hipLaunchKernelGGL((sgd_momentum_kernel<T, false, false>), grid, block, 0, s, xp, gp, m, lr, mu, op, n);
  return check_launch();
}

// S images of n elements each, image-major, over all S * n elements.  A step requests its operands, the old velocity and the
// image's lr / first / active in one batch (no load waits on another); `first` and `active` select where the values are used:
// a first step drops the loaded velocity by a select (it may be NaN: never multiplied into the result), an inactive image
// stores its x back and leaves its velocity alone.  VEC (every base pointer 16-byte aligned and n % N == 0, so every image's
// slice keeps the alignment and no vector spans two images): one 16-byte vector of T per step; otherwise one element per step.
// The element formula is sgd_momentum_kernel's.  x and out may be the same tensor.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void sgd_momentum_batched_kernel(const T* x, const T* __restrict__ g, float* __restrict__ m,
                                                                   const float* __restrict__ lr, float mu,
                                                                   const int* __restrict__ first, const int* __restrict__ active,
                                                                   T* out, long long n, long long total) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  if constexpr (VEC) {
    using P = Pack<T>;
    constexpr int N = P::N;
    for (long long v = tid; v < total / N; v += stride) {
      const typename P::vec xv = reinterpret_cast<const typename P::vec*>(x)[v];
      const typename P::vec gv = reinterpret_cast<const typename P::vec*>(g)[v];
      f32x4* mv = reinterpret_cast<f32x4*>(m) + v * (N / 4);
      f32x4 b[N / 4];
#pragma unroll
      for (int q = 0; q < N / 4; ++q) b[q] = mv[q];
      const long long s = v * N / n;
      const float step = lr[s];
      const int fst = first[s], on = active[s];
      typename P::vec ov;
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float ge = Traits<T>::to_f32(P::get(gv, e));
        const float carried = sgd_velocity(mu, b[e / 4][e % 4], ge);
        const float be = fst ? ge : carried;
        b[e / 4][e % 4] = be;
        P::set(ov, e, sgd_elem<T>(P::get(xv, e), step, be));
      }
      if (on) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) mv[q] = b[q];
      }
      reinterpret_cast<typename P::vec*>(out)[v] = on ? ov : xv;
    }
  } else {
    for (long long i = tid; i < total; i += stride) {
      const T xe = x[i];
      const float ge = Traits<T>::to_f32(g[i]);
      const float bo = m[i];
      const long long s = i / n;
      const float step = lr[s];
      const int fst = first[s], on = active[s];
      const float carried = sgd_velocity(mu, bo, ge);
      const float be = fst ? ge : carried;
      if (on) m[i] = be;
      out[i] = on ? sgd_elem<T>(xe, step, be) : xe;
    }
  }
}

template <typename T>
int do_sgd_momentum_batched(const void* x, const void* g, float* m, const float* lr, float mu, const int* first,
                            const int* active, void* out, int images, long long n, hipStream_t s) {
  const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                     reinterpret_cast<uintptr_t>(out)) & 15) == 0 && n % Pack<T>::N == 0;
  const long long total = (long long)images * n;
  const dim3 grid(grid_for(vec ? total / Pack<T>::N : total)), block(256);
  if (vec)
    hipLaunchKernelGGL((sgd_momentum_batched_kernel<T, true>), grid, block, 0, s, (const T*)x, (const T*)g, m, lr, mu, first,
                       active, (T*)out, n, total);
  else
    hipLaunchKernelGGL((sgd_momentum_batched_kernel<T, false>), grid, block, 0, s, (const T*)x, (const T*)g, m, lr, mu, first,
                       active, (T*)out, n, total);
  return check_launch();
}

template <typename T>
int do_axpy(const void* x, const void* g, float step, void* out, float* absmean, long long n, hipStream_t s) {
  if (absmean)
    hipLaunchKernelGGL(axpy_absmean_kernel<T>, dim3(1), dim3(1024), 0, s, (const T*)x, (const T*)g, step, (T*)out,
                       absmean, n);
  else
    hipLaunchKernelGGL(axpy_kernel<T>, dim3(grid_for(n)), dim3(256), 0, s, (const T*)x, (const T*)g, step, (T*)out, n);
  return check_launch();
}

}  // namespace

extern "C" int ga_latent_axpy(const void* latents, const void* grad, float step, void* out, float* absmean, int64_t n,
                              int dtype, ga_stream_t stream) {
  if (!latents || !grad || !out) return GA_ERR_NULL;
  if (n < 1) return GA_ERR_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case GA_F16:
      return do_axpy<_Float16>(latents, grad, step, out, absmean, n, s);
    case GA_BF16:
      return do_axpy<bf16_t>(latents, grad, step, out, absmean, n, s);
    case GA_F32:
      return do_axpy<float>(latents, grad, step, out, absmean, n, s);
    default:
      return GA_ERR_DTYPE;
  }
}

extern "C" int ga_latent_sgd_momentum(const void* latents, const void* grad, float* momentum, float lr, float mu, int first,
                                      void* out, int64_t n, int dtype, ga_stream_t stream) {
  if (!latents || !grad || !momentum || !out) return GA_ERR_NULL;
  if (n < 1 || !(mu >= 0.f && mu < 1.f)) return GA_ERR_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case GA_F16:
      return do_sgd_momentum<_Float16>(latents, grad, momentum, lr, mu, first, out, n, s);
    case GA_BF16:
      return do_sgd_momentum<bf16_t>(latents, grad, momentum, lr, mu, first, out, n, s);
    case GA_F32:
      return do_sgd_momentum<float>(latents, grad, momentum, lr, mu, first, out, n, s);
    default:
      return GA_ERR_DTYPE;
  }
}

extern "C" int ga_latent_axpby(const void* x, const void* y, float a, float b, void* out, int64_t n, int dtype,
                               ga_stream_t stream) {
  if (!x || !y || !out) return GA_ERR_NULL;
  if (n < 1) return GA_ERR_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(grid_for(n));
  switch (dtype) {
    case GA_F16:
      hipLaunchKernelGGL(axpby_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16*)x, (const _Float16*)y, a, b,
                         (_Float16*)out, (long long)n);
      break;
    case GA_BF16:
      hipLaunchKernelGGL(axpby_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)y, a, b,
                         (bf16_t*)out, (long long)n);
      break;
    case GA_F32:
      hipLaunchKernelGGL(axpby_kernel<float>, grid, dim3(256), 0, s, (const float*)x, (const float*)y, a, b,
                         (float*)out, (long long)n);
      break;
    default:
      return GA_ERR_DTYPE;
  }
  return check_launch();
}

extern "C" int ga_cfg_ddim_step(const void* eps_uncond, const void* eps_text, float guidance, const void* x,
                                float alpha_t, float alpha_prev, void* prev, void* x0_out, int64_t n, int dtype,
                                ga_stream_t stream) {
  if (!eps_uncond || !eps_text || !x || !prev) return GA_ERR_NULL;
  return cfg_ddim_entry(GA_PRED_EPSILON, eps_uncond, eps_text, guidance, x, alpha_t, alpha_prev, nullptr, prev, x0_out, 1, n,
                        dtype, stream);
}

extern "C" int ga_cfg_ddim_step_pred(const void* out_uncond, const void* out_text, float guidance, const void* x, float alpha_t,
                                     float alpha_prev, int prediction, void* prev, void* x0_out, int64_t n, int dtype,
                                     ga_stream_t stream) {
  if (!out_uncond || !out_text || !x || !prev) return GA_ERR_NULL;
  return cfg_ddim_entry(prediction, out_uncond, out_text, guidance, x, alpha_t, alpha_prev, nullptr, prev, x0_out, 1, n, dtype,
                        stream);
}

extern "C" int ga_latent_axpy_batched(const void* latents, const void* grad, const float* step, const int* active,
                                      void* out, float* absmean, int images, int64_t n, int dtype, ga_stream_t stream) {
  if (!latents || !grad || !step || !active || !out) return GA_ERR_NULL;
  if (n < 1 || images < 1 || images > GA_MAX_IMAGES) return GA_ERR_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(images), block(1024);
  switch (dtype) {
    case GA_F16:
      hipLaunchKernelGGL(axpy_batched_kernel<_Float16>, grid, block, 0, s, (const _Float16*)latents, (const _Float16*)grad,
                         step, active, (_Float16*)out, absmean, (long long)n);
      break;
    case GA_BF16:
      hipLaunchKernelGGL(axpy_batched_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)latents, (const bf16_t*)grad, step,
                         active, (bf16_t*)out, absmean, (long long)n);
      break;
    case GA_F32:
      hipLaunchKernelGGL(axpy_batched_kernel<float>, grid, block, 0, s, (const float*)latents, (const float*)grad, step,
                         active, (float*)out, absmean, (long long)n);
      break;
    default:
      return GA_ERR_DTYPE;
  }
  return check_launch();
}

extern "C" int ga_latent_sgd_momentum_batched(const void* latents, const void* grad, float* momentum, const float* lr, float mu,
                                              const int* first, const int* active, void* out, int images, int64_t n,
                                              int dtype, ga_stream_t stream) {
  if (!latents || !grad || !momentum || !lr || !first || !active || !out) return GA_ERR_NULL;
  if (n < 1 || images < 1 || images > GA_MAX_IMAGES || !(mu >= 0.f && mu < 1.f)) return GA_ERR_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case GA_F16:
      return do_sgd_momentum_batched<_Float16>(latents, grad, momentum, lr, mu, first, active, out, images, n, s);
    case GA_BF16:
      return do_sgd_momentum_batched<bf16_t>(latents, grad, momentum, lr, mu, first, active, out, images, n, s);
    case GA_F32:
      return do_sgd_momentum_batched<float>(latents, grad, momentum, lr, mu, first, active, out, images, n, s);
    default:
      return GA_ERR_DTYPE;
  }
}

extern "C" int ga_latent_axpby_masked(const void* x, const void* y, float a, float b, const int* active, void* out,
                                      int images, int64_t n, int dtype, ga_stream_t stream) {
  if (!x || !y || !active || !out) return GA_ERR_NULL;
  if (n < 1 || images < 1 || images > GA_MAX_IMAGES) return GA_ERR_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long total = (long long)images * n;
  const dim3 grid(grid_for(total));
  switch (dtype) {
    case GA_F16:
      hipLaunchKernelGGL(axpby_masked_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16*)x, (const _Float16*)y, a, b,
                         active, (_Float16*)out, (long long)n, total);
      break;
    case GA_BF16:
      hipLaunchKernelGGL(axpby_masked_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)y, a, b,
                         active, (bf16_t*)out, (long long)n, total);
      break;
    case GA_F32:
      hipLaunchKernelGGL(axpby_masked_kernel<float>, grid, dim3(256), 0, s, (const float*)x, (const float*)y, a, b, active,
                         (float*)out, (long long)n, total);
      break;
    default:
      return GA_ERR_DTYPE;
  }
  return check_launch();
}

extern "C" int ga_cfg_ddim_step_masked(const void* eps_uncond, const void* eps_text, float guidance, const void* x,
                                       float alpha_t, float alpha_prev, const int* active, void* prev, void* x0_out,
                                       int images, int64_t n, int dtype, ga_stream_t stream) {
  if (!eps_uncond || !eps_text || !x || !active || !prev) return GA_ERR_NULL;
  return cfg_ddim_entry(GA_PRED_EPSILON, eps_uncond, eps_text, guidance, x, alpha_t, alpha_prev, active, prev, x0_out, images, n,
                        dtype, stream);
}

extern "C" int ga_cfg_ddim_step_pred_masked(const void* out_uncond, const void* out_text, float guidance, const void* x,
                                            float alpha_t, float alpha_prev, int prediction, const int* active, void* prev,
                                            void* x0_out, int images, int64_t n, int dtype, ga_stream_t stream) {
  if (!out_uncond || !out_text || !x || !active || !prev) return GA_ERR_NULL;
  return cfg_ddim_entry(prediction, out_uncond, out_text, guidance, x, alpha_t, alpha_prev, active, prev, x0_out, images, n,
                        dtype, stream);
}

extern "C" int ga_cfg_ddim_step_eta(const void* out_uncond, const void* out_text, float guidance, const void* x,
                                    const void* noise, float alpha_t, float alpha_prev, float eta, int prediction, void* prev,
                                    void* x0_out, int64_t n, int dtype, ga_stream_t stream) {
  if (!out_uncond || !out_text || !x || !prev || (eta > 0.f && !noise)) return GA_ERR_NULL;
  return cfg_ddim_eta_entry(prediction, out_uncond, out_text, guidance, x, noise, alpha_t, alpha_prev, eta, nullptr, prev, x0_out,
                            1, n, dtype, stream);
}

extern "C" int ga_cfg_ddim_step_eta_masked(const void* out_uncond, const void* out_text, float guidance, const void* x,
                                           const void* noise, float alpha_t, float alpha_prev, float eta, int prediction,
                                           const int* active, void* prev, void* x0_out, int images, int64_t n, int dtype,
                                           ga_stream_t stream) {
  if (!out_uncond || !out_text || !x || !active || !prev || (eta > 0.f && !noise)) return GA_ERR_NULL;
  return cfg_ddim_eta_entry(prediction, out_uncond, out_text, guidance, x, noise, alpha_t, alpha_prev, eta, active, prev, x0_out,
                            images, n, dtype, stream);
}

// ga_latent_affine4: the VAE decoder's `latents / scaling_factor` and its 4 -> 4 post_quant_conv (1x1) in one pass over dense
// NCHW [B][4][hw]: out[b][o][p] = bias[o] + sum_i W[o][i] * (pre_scale * x[b][i][p]), f32 fmas in the order i = 0..3.
namespace {

template <typename T>
__global__ __launch_bounds__(256) void latent_affine4_kernel(const T* __restrict__ x, const T* __restrict__ W,
                                                             const T* __restrict__ bias, float pre_scale, T* __restrict__ out,
                                                             long long hw, long long pixels) {
  float w[4][4], bv[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    bv[o] = Traits<T>::to_f32(bias[o]);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[o][i] = Traits<T>::to_f32(W[o * 4 + i]);
  }
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < pixels; t += (long long)gridDim.x * 256) {
    const long long b = t / hw, p = t - b * hw;
    const T* xp = x + b * 4 * hw + p;
    T* op = out + b * 4 * hw + p;
    float xs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xs[i] = pre_scale * Traits<T>::to_f32(xp[i * hw]);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float acc = bv[o];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = __fmaf_rn(w[o][i], xs[i], acc);
      op[o * hw] = Traits<T>::from_f32(acc);
    }
  }
}

template <typename T>
int do_affine4(const void* x, const void* W, const void* bias, float pre_scale, void* out, int B, long long hw, hipStream_t s) {
  const long long pixels = (long long)B * hw;
  hipLaunchKernelGGL(latent_affine4_kernel<T>, dim3(grid_for(pixels)), dim3(256), 0, s, (const T*)x, (const T*)W,
                     (const T*)bias, pre_scale, (T*)out, hw, pixels);
  return check_launch();
}

}  // namespace

extern "C" int ga_latent_affine4(const void* x, const void* W, const void* bias, float pre_scale, void* out, int B, int64_t hw,
                                 int dtype, ga_stream_t stream) {
  if (!x || !W || !bias || !out) return GA_ERR_NULL;
  if (B < 1 || hw < 1 || hw > (int64_t)1 << 40) return GA_ERR_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case GA_F16: return do_affine4<_Float16>(x, W, bias, pre_scale, out, B, hw, s);
    case GA_BF16: return do_affine4<bf16_t>(x, W, bias, pre_scale, out, B, hw, s);
    case GA_F32: return do_affine4<float>(x, W, bias, pre_scale, out, B, hw, s);
    default: return GA_ERR_DTYPE;
  }
}

extern "C" int ga_version(void) { return GA_VERSION; }

extern "C" const char* ga_strerror(int status) {
  switch (status) {
    case GA_OK: return "ok";
    case GA_ERR_NULL: return "required pointer is NULL";
    case GA_ERR_SHAPE: return "size out of the supported range";
    case GA_ERR_DTYPE: return "unknown dtype";
    case GA_ERR_ALIGN: return "pointer not 16-byte aligned or head_dim not a multiple of 8";
    case GA_ERR_LAUNCH: return "kernel launch failed";
    case GA_ERR_UNSUPPORTED: return "not implemented in this build";
    default: return "unknown status";
  }
}
