// Forward-only flash attention for wide heads: 64 <= D <= 512, D % 64 == 0 — the VAE decoder's mid-block attention (one head
// of 512 channels over H*W tokens, vae.py), which the kernels of self_attn.hip (D <= 160) do not reach.
//
//   O = softmax(scale Q K^T) V,   Q, K, V, O [B][N][H][D] (ld_qkv as for ga_self_attn_fwd), no LSE, no backward.
//
// Same transposed-score mapping as self_attn.hip: a workgroup of four waves owns 64 queries of one (batch, head), a wave 16 of
// them ON ITS LANES (lane c = query, g = lane >> 4).  S^T = K Q^T puts the keys on accumulator rows, so the softmax of a
// lane's query is in-lane plus two cross-lane steps, and the probabilities are already the B operand of O^T = V^T P^T.
// The whole O^T tile of a wave (D x 16 f32: D / 4 registers per lane, 128 at D = 512) and its Q fragments (D / 8 registers)
// stay in registers; the build keeps MFMA results in VGPRs and a 256-thread workgroup runs one wave per SIMD (512 VGPRs).
// Key tiles are 32 keys: K row-major with the bank-padded stride of TileLds, V row-major with the odd-multiple-of-16 stride
// the transposing read needs (trs), double-buffered — 2 x (32 x 520 + 32 x 528) x 2 B = 131 KB at D = 512.  The next tile is
// loaded to registers before the current tile's math and written to the other buffer after it: one barrier per tile.
// Scores, the running maximum and sum are f32; P is rounded to T for the second MFMA as in self_attn.hip; O is rounded once,
// at its store.  Throughput is not the point of this kernel (34 GFLOP for the 4096-token mid block of a 512^2 image).
#include "attn_common.h"

using namespace ga;

namespace {

constexpr int kThreads = 256;  // 4 waves x 16 queries
constexpr int kKT = 32;        // keys per tile

template <int NK>
__host__ __device__ constexpr int wide_buf_elems() {
  return kKT * (NK * 16 + 8) + kKT * trs<NK>();
}

template <typename T, int NK>
__global__ __launch_bounds__(kThreads) void attn_wide_fwd_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                                 const T* __restrict__ V, T* __restrict__ O, int H, int N,
                                                                 int nqt, int ldq, float scale_log2) {
  using Tr = Traits<T>;
  static_assert(sizeof(T) == 2 && NK % 4 == 0, "16-bit types, head sizes that are multiples of 64");
  constexpr int D = NK * 16;
  constexpr int KS = D + 8;              // K image row stride (TileLds::ks)
  constexpr int VS = trs<NK>();          // V image row stride (transposing read)
  constexpr int kVoff = kKT * KS;
  constexpr int kBuf = wide_buf_elems<NK>();
  constexpr int VPR = D / 8;             // 16-byte vectors per row
  constexpr int PER = kKT * VPR / kThreads;   // vectors per thread and matrix (= D / 64)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* const lds = reinterpret_cast<T*>(smem);

  // head-fastest workgroup order: the workgroups that sweep one head's K / V follow each other
  const int head = blockIdx.x % H;
  const int rest = blockIdx.x / H;
  const int qt = rest % nqt, b = rest / nqt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const size_t rs = (size_t)ldq, rso = (size_t)H * D;
  const T* Qb = Q + (size_t)b * N * rs + (size_t)head * D;
  const T* Kb = K + (size_t)b * N * rs + (size_t)head * D;
  const T* Vb = V + (size_t)b * N * rs + (size_t)head * D;
  const int q0 = qt * 64 + wave * 16;

  // this lane's Q fragments: row min(q, N - 1) (a lane past the sequence computes on a valid row and stores nothing)
  typename Tr::frag qf[NK];
  {
    const T* qrow = Qb + (size_t)min(q0 + c, N - 1) * rs + 4 * g;
#pragma unroll
    for (int kc = 0; kc < NK; ++kc) qf[kc] = load_frag<T>(qrow + kc * 16);
  }

  // staging registers of one tile: rows are clamped into the sequence for the load and zeroed at the LDS store where they
  // lie past it (a V row past N meets a zero probability, and 0 x garbage must stay 0)
  uint4 kv[PER], vv[PER];
  auto stage_load = [&](int k0) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = u * kThreads + threadIdx.x;
      const int r = idx / VPR, d = (idx - r * VPR) * 8;
      const size_t off = (size_t)min(k0 + r, N - 1) * rs + d;
      kv[u] = *reinterpret_cast<const uint4*>(Kb + off);
      vv[u] = *reinterpret_cast<const uint4*>(Vb + off);
    }
  };
  auto stage_store = [&](T* buf, int k0) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = u * kThreads + threadIdx.x;
      const int r = idx / VPR, d = (idx - r * VPR) * 8;
      const bool live = k0 + r < N;
      *reinterpret_cast<uint4*>(buf + r * KS + d) = live ? kv[u] : uint4{0, 0, 0, 0};
      *reinterpret_cast<uint4*>(buf + kVoff + r * VS + d) = live ? vv[u] : uint4{0, 0, 0, 0};
    }
  };

  f32x4 o[NK];
#pragma unroll
  for (int dt = 0; dt < NK; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;   // running maximum (log2 domain) of this lane's query; this lane's share of the row sum

  const int ntiles = (N + kKT - 1) / kKT;
  stage_load(0);
  stage_store(lds, 0);
  __syncthreads();
  for (int kt = 0; kt < ntiles; ++kt) {
    const bool more = kt + 1 < ntiles;   // workgroup-uniform
    if (more) stage_load((kt + 1) * kKT);
    const T* kimg = lds + (kt & 1) * kBuf;
    const T* vimg = kimg + kVoff;

    // scores of 32 keys x 16 queries: keys on accumulator rows (lane (c, g) holds keys rb * 16 + 4 g + i of query c)
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const T* krow = kimg + c * KS + 4 * g;
#pragma unroll
    for (int kc = 0; kc < NK; kc += 2)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        const typename Tr::frag a0 = lds_frag<T>(krow + rb * 16 * KS + kc * 16);
        const typename Tr::frag a1 = lds_frag<T>(krow + rb * 16 * KS + kc * 16 + 16);
        s[rb] = Tr::mma16x2(a0, a1, qf[kc], qf[kc + 1], s[rb]);
      }
    const int key0 = kt * kKT;
    float tmax = -INFINITY;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float x = s[rb][i] * scale_log2;
        if (key0 + rb * 16 + 4 * g + i >= N) x = -INFINITY;   // every tile holds at least one live key
        s[rb][i] = x;
        tmax = fmaxf(tmax, x);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax);
    if (__builtin_amdgcn_ballot_w64(m_new > m) != 0) {   // wave-uniform: some query's maximum moved
      const float alpha = exp2f(m - m_new);              // the first tile: exp2(-inf) = 0 on o = l = 0
      l *= alpha;
#pragma unroll
      for (int dt = 0; dt < NK; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) o[dt][i] *= alpha;
      m = m_new;
    }
    typename Tr::frag pf[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = exp2f(s[rb][i] - m);
        l += p;
        pf[rb][i] = Tr::from_f32(p);
      }
    // O^T[d][query] += V^T[d][keys] P^T[keys][query]: V stays row-major and is read transposed (see rowsT_times_frags in
    // self_attn.hip for the lane -> address map); every feature block is its own accumulator chain.  EXEC is all ones here.
    const T* vbase = vimg + (4 * g + (c >> 2)) * VS + 4 * (c & 3);
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) {
      const typename Tr::frag a0 = tr_read<T>(vbase + dt * 16);
      const typename Tr::frag a1 = tr_read<T>(vbase + 16 * VS + dt * 16);
      o[dt] = Tr::mma16x2(a0, a1, pf[0], pf[1], o[dt]);
    }
    if (more) stage_store(lds + ((kt + 1) & 1) * kBuf, (kt + 1) * kKT);   // free since the barrier that ended tile kt - 1
    __syncthreads();
  }

  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.0f / l;
  const int q = q0 + c;
  if (q < N) {
    T* orow = O + ((size_t)b * N + q) * rso + (size_t)head * D + 4 * g;   // lane (c, g) holds features dt * 16 + 4 g + i
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) {
      typename Tr::frag f;
#pragma unroll
      for (int i = 0; i < 4; ++i) f[i] = Tr::from_f32(o[dt][i] * inv);
      store_frag<T>(orow + dt * 16, f);
    }
  }
}

struct WideCall {
  const void *Q, *K, *V;
  void* O;
  int B, H, N, ldq;
  float scale_log2;
  hipStream_t stream;
};

template <typename T, int NK>
int launch_wide(const WideCall& c) {
  const size_t bytes = 2 * (size_t)wide_buf_elems<NK>() * sizeof(T);
  int rc = set_dyn_lds(attn_wide_fwd_kernel<T, NK>, bytes);
  if (rc != GA_OK) return rc;
  const int nqt = (c.N + 63) / 64;
  hipLaunchKernelGGL((attn_wide_fwd_kernel<T, NK>), dim3((unsigned)((size_t)c.B * c.H * nqt)), dim3(kThreads), bytes, c.stream,
                     (const T*)c.Q, (const T*)c.K, (const T*)c.V, (T*)c.O, c.H, c.N, nqt, c.ldq, c.scale_log2);
  return check_launch();
}

template <typename T>
int by_width(const WideCall& c, int D) {
  switch (D / 64) {
    case 1: return launch_wide<T, 4>(c);
    case 2: return launch_wide<T, 8>(c);
    case 3: return launch_wide<T, 12>(c);
    case 4: return launch_wide<T, 16>(c);
    case 5: return launch_wide<T, 20>(c);
    case 6: return launch_wide<T, 24>(c);
    case 7: return launch_wide<T, 28>(c);
    case 8: return launch_wide<T, 32>(c);
    default: return GA_ERR_SHAPE;
  }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int ga_attn_wide_fwd(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D, int ld_qkv,
                                float scale, int dtype, ga_stream_t stream) {
  if (!Q || !K || !V || !O) return GA_ERR_NULL;
  if (dtype != GA_F16 && dtype != GA_BF16 && dtype != GA_F32) return GA_ERR_DTYPE;
  if (B <= 0 || H <= 0 || N <= 0 || D < 64 || D > 512 || D % 64 != 0) return GA_ERR_SHAPE;
  if (ld_qkv != 0 && (long long)ld_qkv != 3LL * H * D) return GA_ERR_SHAPE;
  if ((long long)B * H * ((N + 63) / 64) > 0x7fffffffLL || 3LL * H * D > 0x7fffffffLL) return GA_ERR_SHAPE;
  if (dtype == GA_F32) return GA_ERR_UNSUPPORTED;
  if (!al16(Q) || !al16(K) || !al16(V) || !al16(O)) return GA_ERR_ALIGN;
  WideCall c{Q, K, V, O, B, H, N, ld_qkv ? ld_qkv : H * D, scale * 1.4426950408889634f, static_cast<hipStream_t>(stream)};
  return dtype == GA_F16 ? by_width<_Float16>(c, D) : by_width<bf16_t>(c, D);
}
