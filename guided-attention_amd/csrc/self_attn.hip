// Tiled (flash-style) attention for long key sequences — the UNet's self-attention layers (N = 64 ... 4096
// keys) inside the same attention processor (utils/ptp_utils.py:66-146 with encoder_hidden_states = None).
// The reference materialises P = softmax(scale Q K^T) as an (8, 4096, 4096) tensor per 64x64 layer (268 MB in
// fp16, x5 layers, kept alive by autograd); here P never leaves the registers.
//
//   forward  : O = softmax(scale Q K^T) V, plus LSE (per query, log2 domain) for the backward
//   backward : recompute-based, two kernels without atomics (deterministic; delta is taken in the first one):
//                dq    : per query block, sweeps the key tiles:  dQ  = scale * sum_k dS K
//                dk_dv : per key block, sweeps the query tiles:  dV = P^T dO,  dK = scale * dS^T Q
//              with dS = P o (dO V^T - delta), delta = rowsum(dO o O) (taken by the dq kernel from its own fragments).
//              With a cotangent dP on the probabilities (ga_self_attn_bwd_dp): dS = P o (dO V^T + dP - delta - r),
//              r = rowsum(P o dP) from a row pre-pass, then the same two kernel bodies with the dP tile in the dp chain.
//
// gfx950 mapping (same transposed-score trick as attn_capture.hip): a wave owns QB x 16 queries (dq / forward) or
// QB x 16 keys (dk_dv) ON ITS LANES; the swept tile (64 rows) sits in LDS as a bank-padded row-major image and/or a
// bank-rotated transposed image, double-buffered, next tile prefetched to registers while the current one feeds
// v_mfma_f32_16x16x16 (f16 / bf16; exact-f32 v_mfma_f32_16x16x4 for the f32 build).  Keys (or queries) land on
// accumulator rows, so the softmax statistics of a lane's column are in-lane + two cross-lane steps, and every
// accumulator tile that feeds a second contraction (P -> PV, dS -> dQ / dK, P -> dV) is already in B-operand
// layout: no LDS round trip between chained MFMAs.  Tensors stay in the projection layout [B][N][H][D].
// Workgroup ids run head-fastest so that, with 8 heads and round-robin XCD dispatch, the workgroups that sweep one
// head's K/V share an XCD L2.   MFMA-bound for N >= 1024 (4 N^2 D flops per head forward), latency-bound below.
#include <cstdlib>
#include "attn_common.h"

using namespace ga;

namespace {

constexpr int kThreads = 256;  // 4 waves

// KT = rows of the swept tile (keys in fwd / dq, queries in dk_dv): 64, or 128 where the registers allow it
// (fewer barriers and loop overheads per key: the 16-query forward ran 111 -> 91 us on the 4096-token layer).
template <typename T, int KT>
using TL = TileLds<T, KT>;

// ---- staging: [rows][D] slice of a [B][N][H][D] tensor -> registers -> LDS images -------------------------------
// V16 = 16-byte vectors per thread and matrix for one 64-row tile (DP*64 / VEC / 256)
// PRE = true keeps the per-lane global addresses in registers (computed once; full tiles load without exec-mask
// branches): fastest where registers are free (forward).  PRE = false recomputes them per tile and costs no
// registers: the backward kernels sit at the VGPR limit and lost 15 % with the resident addresses.
template <typename T, int NK, int KT, bool PRE, int NT = kThreads>
struct Stage {
  static constexpr int VEC = TL<T, KT>::VEC;
  static constexpr int DP = NK * 16;
  static constexpr int VPR = DP / VEC;                                    // vectors per row
  static constexpr int TOTAL = KT * VPR;                                  // vectors per tile
  static constexpr int PER = (TOTAL + NT - 1) / NT;           // vectors per thread
  static constexpr int NP = PRE ? PER : 1;
  uint4 v[PER];
  const T* base;      // the [rows][D] slice (wave-uniform: the loads take it as their scalar base)
  unsigned off[NP];   // PRE: byte offset of this lane's vector u inside tile 0, clamped in-bounds for idle lanes
  int aux[NP];        // PRE: row inside the tile, -1 = idle lane; else aux[0] = D
  int tile_row0, seq_rows;   // !PRE: first row of the tile in flight and the sequence length (uniform), for value()

  __device__ __forceinline__ void init(const T* __restrict__ slice, int D, size_t row_stride) {
    base = slice;
    if (PRE) {
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int idx = u * NT + (threadIdx.x & (NT - 1));
        const int r = idx / VPR, d = (idx - r * VPR) * VEC;
        const bool live = idx < TOTAL && d < D;
        // Idle lanes (the columns D..DP of a row, or beyond the tile) read a valid vector of the same tile instead:
        // no select on the address, and what they put into the pad columns is finite data that only ever meets the
        // zero pad of the other MFMA operand or lands in output columns that are never stored.
        const int rc = r < KT ? r : KT - 1, dc = d < D ? d : D - VEC;
        aux[u < NP ? u : 0] = live ? r : -1;
        off[u < NP ? u : 0] = (unsigned)(((size_t)rc * row_stride + dc) * sizeof(T));
      }
    } else {
      aux[0] = D;
    }
  }
  __device__ __forceinline__ void load(int row0, int N, size_t row_stride) {
    if (PRE) {
      // buffer loads: descriptor (slice base) and tile offset in scalar registers, the lane's 32-bit offset in one
      // VGPR — no 64-bit address arithmetic per load
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      const __amdgpu_buffer_rsrc_t rsrc =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), 0, 0x7FFFFFFF, 0x00020000);
      const unsigned tile = (unsigned)((size_t)row0 * row_stride * sizeof(T));  // scalar
      if (row0 + KT <= N) {
        // full tile: unconditional loads and NOTHING that consumes the data here — a select on the loaded value in
        // this block makes the compiler wait for the load on the spot (s_waitcnt vmcnt(0) before the tile's math:
        // the prefetch is then no prefetch)
#pragma unroll
        for (int u = 0; u < PER; ++u) {
          const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off[u < NP ? u : 0], tile, 0);
          v[u] = uint4{x[0], x[1], x[2], x[3]};
        }
      } else {  // the last, partial tile: rows beyond N must be zero (V rows meet live P columns)
#pragma unroll
        for (int u = 0; u < PER; ++u) {
          const int i = u < NP ? u : 0;
          v[u] = uint4{0, 0, 0, 0};
          if (aux[i] >= 0 && row0 + aux[i] < N) {
            const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off[i], tile, 0);
            v[u] = uint4{x[0], x[1], x[2], x[3]};
          }
        }
      }
    } else if constexpr (sizeof(T) == 4 && NK > 5) {   // fp32 at head sizes > 80: register budget (no UNet here runs it)
      const int D = aux[0];
      tile_row0 = 0;
      seq_rows = 1 << 30;   // value(): what was not loaded is already zero
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int idx = u * NT + (threadIdx.x & (NT - 1));
        const int r = idx / VPR, d = (idx - r * VPR) * VEC;
        v[u] = uint4{0, 0, 0, 0};
        if (idx < TOTAL && row0 + r < N && d < D)
          v[u] = *reinterpret_cast<const uint4*>(base + (size_t)(row0 + r) * row_stride + d);
      }
    } else {
      // Unconditional loads from (row, column) clamped into the slice; what is dead (beyond the tile, the sequence or the
      // head size) becomes zero in value(), where the data is consumed.  With the load under the condition every vector
      // sat in a block of its own behind a wait: the "prefetch" of the backward kernels was one round trip per vector.
      const int D = aux[0];
      tile_row0 = row0;
      seq_rows = N;
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int idx = u * NT + (threadIdx.x & (NT - 1));
        const int r = idx / VPR, d = (idx - r * VPR) * VEC;
        const int rc = min(row0 + min(r, KT - 1), N - 1), dc = min(d, D - VEC);
        v[u] = *reinterpret_cast<const uint4*>(base + (size_t)rc * row_stride + dc);
      }
    }
  }
  __device__ __forceinline__ uint4 value(int u) const {
    if constexpr (PRE || (sizeof(T) == 4 && NK > 5)) {
      return v[u];
    } else {
      const int idx = u * NT + (threadIdx.x & (NT - 1));
      const int r = idx / VPR, d = (idx - r * VPR) * VEC;
      const bool live = idx < TOTAL && tile_row0 + r < seq_rows && d < aux[0];
      return live ? v[u] : uint4{0, 0, 0, 0};
    }
  }
  // ones_d >= 0: the 16-byte vector that starts at column ones_d (the first pad vector of a head size that is not a
  // multiple of 16) is stored as {1, 0, 0, ...} instead of what was loaded: a column of ones in the V image makes the
  // P.V product deliver the softmax row sum in output row ones_d — no VALU adds for it (forward, 16-bit types).
  template <int STRIDE>
  __device__ __forceinline__ void store_rows(T* img, int ones_d = -1) const {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = u * NT + (threadIdx.x & (NT - 1));
      if (idx >= TOTAL) continue;
      const int r = idx / VPR, d = (idx - r * VPR) * VEC;
      uint4 val = value(u);
      if (d == ones_d) val = uint4{sizeof(T) == 2 ? (Traits<T>::kDtype == GA_F16 ? 0x3C00u : 0x3F80u) : 0x3F800000u, 0, 0, 0};
      *reinterpret_cast<uint4*>(img + r * STRIDE + d) = val;
    }
  }
  // the row-major image with every element stored as round_T(x * f): what scale_frags makes of a register fragment
  __device__ __forceinline__ void store_scaled(T* rowmaj, float f) const {
    constexpr int KS = DP + VEC;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = u * NT + (threadIdx.x & (NT - 1));
      if (idx >= TOTAL) continue;
      const int r = idx / VPR, d = (idx - r * VPR) * VEC;
      uint4 val = value(u);
      if constexpr (Traits<T>::kDtype == GA_F16) {
        // v_fma_mix: f16 half -> f32, x f (rounded to f32), -> f16, written back into the half it came from — the value of
        // (_Float16)((float)x * f) (a zero comes out +0) in one instruction per element and no temporary register (the
        // head-size-160 kernels have none to spare: with separate conversions the compiler spilled).  f is wave-uniform.
        unsigned* w = reinterpret_cast<unsigned*>(&val);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          asm("v_fma_mixlo_f16 %0, %0, %1, 0 op_sel_hi:[1,0,0]\n\t"
              "v_fma_mixhi_f16 %0, %0, %1, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
              : "+v"(w[j])
              : "s"(f));
      } else {
        typename Traits<T>::frag* fr = reinterpret_cast<typename Traits<T>::frag*>(&val);   // 16 bytes = VEC / 4 fragments
#pragma unroll
        for (int h = 0; h < VEC / 4; ++h)
#pragma unroll
          for (int i = 0; i < 4; ++i) fr[h][i] = Traits<T>::from_f32(Traits<T>::to_f32(fr[h][i]) * f);
      }
      *reinterpret_cast<uint4*>(rowmaj + r * KS + d) = val;
    }
  }
  __device__ __forceinline__ void store(T* rowmaj, T* transposed) const {
    constexpr int KS = DP + VEC;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = u * NT + (threadIdx.x & (NT - 1));
      if (idx >= TOTAL) continue;
      const int r = idx / VPR, d = (idx - r * VPR) * VEC;
      const uint4 val = value(u);
      if (rowmaj) *reinterpret_cast<uint4*>(rowmaj + r * KS + d) = val;
      if (transposed) {
        const T* e = reinterpret_cast<const T*>(&val);
#pragma unroll
        for (int i = 0; i < VEC; ++i) transposed[TL<T, KT>::tr(d + i) + r] = e[i];
      }
    }
  }
};

template <typename T, int NK, int KT>
__host__ __device__ constexpr int row_img() { return KT * (NK * 16 + TL<T, KT>::VEC); }
template <typename T, int NK, int KT>
__host__ __device__ constexpr int tr_img() {
  return NK * 16 * TL<T, KT>::VS + TL<T, KT>::ROT * (NK * 16 / TL<T, KT>::VEC);
}

// acc[rb][cb] += Img[rb*16 + .][:] . X[cb][:]   (rows of the LDS image on accumulator rows, this lane's column
// fragments X in registers);  NRB row blocks of 16, CB column blocks.  k-chunks go through the MFMA in pairs
// (16x16x32: twice the work of a 16x16x16 in the same cycles).
// One row block's fragments: NK chunks, plus (16-bit types, odd NK) the chunk-0 fragment once more as the finite
// filler that pairs with the odd chunk.
template <typename T, int NK>
struct RowFrags {
  static constexpr int NF = (sizeof(T) == 2 && (NK & 1)) ? NK + 1 : NK;
  typename Traits<T>::frag a[NF];
  __device__ __forceinline__ void load(const T* row) {
#pragma unroll
    for (int kc = 0; kc < NK; ++kc) a[kc] = lds_frag<T>(row + kc * 16);
    if (NF > NK) a[NF - 1] = lds_frag<T>(row);
  }
};

// AHEAD = how many row blocks' reads are in flight before the first MFMA: 1 = depth-2 software pipeline (the reads of
// row block rb + 1 fly while rb's MFMAs issue; cheap in registers), NRB = the whole tile up front (the LDS latency
// is paid once per tile instead of once per row block; 2 VGPRs per fragment).  The compiler, left alone, reuses one
// register set and exposes the latency every row block.
// INIT: the first k-step of every row block takes init[cb] (ROWINIT: init_rows[rb], one value per accumulator row) as its
// C operand instead of acc — row constants such as -max, -LSE or -delta enter through the MFMA for free, and acc needs
// no zeroing.
template <typename T, int NK, int NRB, int CB, int AHEAD = 1, bool INIT = false, bool ROWINIT = false>
__device__ __forceinline__ void rows_times_cols(const T* img, const typename Traits<T>::frag (&x)[CB][NK], int c, int g,
                                                f32x4 (&acc)[NRB][CB], const f32x4* init = nullptr,
                                                const f32x4* init_rows = nullptr) {
  constexpr int KS = NK * 16 + TileLds<T, 64>::VEC;
  constexpr int NS = AHEAD + 1 < NRB ? AHEAD + 1 : NRB;  // fragment register sets
  const typename Traits<T>::frag z = zero_frag<T>();
  const T* row0 = img + c * KS + 4 * g;
  RowFrags<T, NK> fr[NS];
#pragma unroll
  for (int rb = 0; rb < AHEAD && rb < NRB; ++rb) fr[rb % NS].load(row0 + rb * 16 * KS);
  // one k-step of one row block; an odd last chunk of a 16-bit type is the same 16x16x32 with the column operand's
  // upper half zero (loop-invariant registers) and, on the row side, the chunk-0 fragment once more as a finite
  // filler — no zeroing moves in the loop.  Do NOT chain a legacy v_mfma_f32_16x16x16_f16 onto a 16x16x32's
  // accumulator: hipcc (ROCm 7.2) emits the pair back-to-back without the wait states the differing pass counts
  // need, and the second MFMA reads a stale SrcC (wrong results).
  auto step = [&](int rb, int kc) {
    const RowFrags<T, NK>& f = fr[rb % NS];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const f32x4 cin = (INIT && kc == 0) ? (ROWINIT ? init_rows[rb] : init[cb]) : acc[rb][cb];
      if (kc + 1 < NK) {
        acc[rb][cb] = Traits<T>::mma16x2(f.a[kc], f.a[kc + 1], x[cb][kc], x[cb][kc + 1], cin);
      } else if constexpr ((NK & 1) != 0) {  // the odd last chunk
        constexpr int L = RowFrags<T, NK>::NF - 1;  // index of the filler (16-bit types)
        if constexpr (sizeof(T) == 2) acc[rb][cb] = Traits<T>::mma16x2(f.a[NK - 1], f.a[L], x[cb][NK - 1], z, cin);
        else acc[rb][cb] = Traits<T>::mma16(f.a[NK - 1], x[cb][NK - 1], cin);
      }
    }
  };
  if constexpr (AHEAD >= NRB) {
    // every fragment is already on its way: sweep the k-steps over batches of 4 row blocks, so that an MFMA never
    // waits for the one issued just before it (the two k-steps of a row block are a dependent chain)
    constexpr int GRP = NRB < 4 ? NRB : 4;
#pragma unroll
    for (int rb0 = 0; rb0 < NRB; rb0 += GRP)
#pragma unroll
      for (int kc = 0; kc < NK; kc += 2)
#pragma unroll
        for (int rb = rb0; rb < rb0 + GRP && rb < NRB; ++rb) step(rb, kc);
  } else {
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      if (rb + AHEAD < NRB) fr[(rb + AHEAD) % NS].load(row0 + (rb + AHEAD) * 16 * KS);
#pragma unroll
      for (int kc = 0; kc < NK; kc += 2) step(rb, kc);
    }
  }
}

// out[dt][cb] += ImgT[dt*16 + .][rows] . F[rb][cb]   (transposed image rows = feature d; contraction over the
// tile rows; F = accumulator tiles converted to operand fragments)
template <typename T, int NK, int NRB, int CB>
__device__ __forceinline__ void featT_times_frags(const T* imgT, const typename Traits<T>::frag (&f)[NRB][CB], int c,
                                                  int g, f32x4 (&out)[NK][CB]) {
  static_assert(NRB % 2 == 0, "row blocks are consumed in pairs");
#pragma unroll
  for (int dt = 0; dt < NK; ++dt) {
    const T* row = imgT + TL<T, NRB * 16>::tr(dt * 16 + c) + 4 * g;
#pragma unroll
    for (int rb = 0; rb < NRB; rb += 2) {
      const typename Traits<T>::frag a0 = load_frag<T>(row + rb * 16), a1 = load_frag<T>(row + rb * 16 + 16);
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) out[dt][cb] = Traits<T>::mma16x2(a0, a1, f[rb][cb], f[rb + 1][cb], out[dt][cb]);
    }
  }
}

// The same product from a ROW-major [tile row][TRS] image through the transposing read (16-bit types): lane
// 16 grp + 4 q + p addresses row 4 grp + q of the 16-row block, columns 4p..4p+3 of the 16-feature block, and
// receives feature (lane & 15) of rows 4 grp .. 4 grp + 3 — the A fragment of the MFMA.  EXEC must be all ones.
template <typename T, int NK, int NRB, int CB>
__device__ __forceinline__ void rowsT_times_frags(const T* img, const typename Traits<T>::frag (&f)[NRB][CB], int lane,
                                                  f32x4 (&out)[NK][CB]) {
  static_assert(NRB % 2 == 0, "row blocks are consumed in pairs");
  constexpr int S = trs<NK>();
  const int i = lane & 15;
  const T* base = img + (4 * (lane >> 4) + (i >> 2)) * S + 4 * (i & 3);
  // depth-2 pipeline over pairs of row blocks; inside a stage the NK feature blocks are independent accumulator
  // chains, so consecutive MFMAs never wait on each other
  typename Traits<T>::frag a[2][NK][2];
  auto load = [&](int st, int rb) {
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) {
      a[st][dt][0] = tr_read<T>(base + rb * 16 * S + dt * 16);
      a[st][dt][1] = tr_read<T>(base + (rb + 1) * 16 * S + dt * 16);
    }
  };
  load(0, 0);
#pragma unroll
  for (int rb = 0; rb < NRB; rb += 2) {
    const int st = (rb >> 1) & 1;
    if (rb + 2 < NRB) load(st ^ 1, rb + 2);
    __builtin_amdgcn_sched_barrier(0);  // keep the next stage's reads ahead of this stage's MFMAs
#pragma unroll
    for (int dt = 0; dt < NK; ++dt)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
        out[dt][cb] = Traits<T>::mma16x2(a[st][dt][0], a[st][dt][1], f[rb][cb], f[rb + 1][cb], out[dt][cb]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The same product with ALL of the tile's transposing reads issued first (load) and the MFMAs later (apply): the
// forward puts its softmax between the two, so the reads land under VALU work instead of in front of the MFMAs.
template <typename T, int NK, int NRB>
struct ColFrags {
  typename Traits<T>::frag a[NRB / 2][NK][2];
  __device__ __forceinline__ void load(const T* img, int lane) {
    constexpr int S = trs<NK>();
    const int i = lane & 15;
    const T* base = img + (4 * (lane >> 4) + (i >> 2)) * S + 4 * (i & 3);
#pragma unroll
    for (int rb = 0; rb < NRB; rb += 2)
#pragma unroll
      for (int dt = 0; dt < NK; ++dt) {
        a[rb >> 1][dt][0] = tr_read<T>(base + rb * 16 * S + dt * 16);
        a[rb >> 1][dt][1] = tr_read<T>(base + (rb + 1) * 16 * S + dt * 16);
      }
    __builtin_amdgcn_sched_barrier(0);  // the reads stay here, ahead of whatever follows
  }
  template <int CB>
  __device__ __forceinline__ void apply(const typename Traits<T>::frag (&f)[NRB][CB], f32x4 (&out)[NK][CB]) const {
#pragma unroll
    for (int rb = 0; rb < NRB; rb += 2)
#pragma unroll
      for (int dt = 0; dt < NK; ++dt)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
          out[dt][cb] = Traits<T>::mma16x2(a[rb >> 1][dt][0], a[rb >> 1][dt][1], f[rb][cb], f[rb + 1][cb], out[dt][cb]);
  }
};

// elements of the image that feeds rowsT / featT products
template <typename T, int NK, int KT>
__host__ __device__ constexpr int col_img() {
  return kTrRead<T> ? KT * trs<NK>() : tr_img<T, NK, KT>();
}

// stage one tile into the image read by rows (may be null) and the image read by columns
template <typename T, int NK, int KT, bool PRE, int NT>
__device__ __forceinline__ void store_tile(const Stage<T, NK, KT, PRE, NT>& st, T* row_image, T* col_image, int ones_d = -1) {
  if constexpr (kTrRead<T>) {
    if (row_image) st.store(row_image, nullptr);
    st.template store_rows<trs<NK>()>(col_image, ones_d);
  } else {
    st.store(row_image, col_image);
  }
}

// out[dt][cb] += (tile rows as the contraction index) ^T . F[rb][cb], from whichever column image the type uses
template <typename T, int NK, int NRB, int CB>
__device__ __forceinline__ void tileT_times_frags(const T* col_image, const typename Traits<T>::frag (&f)[NRB][CB],
                                                  int lane, f32x4 (&out)[NK][CB]) {
  if constexpr (kTrRead<T>) rowsT_times_frags<T, NK, NRB, CB>(col_image, f, lane, out);
  else featT_times_frags<T, NK, NRB, CB>(col_image, f, lane & 15, lane >> 4, out);
}

template <typename T, int NK, int CB>
__device__ __forceinline__ void load_col_frags(const T* __restrict__ base, size_t row_stride, int row0, int N, int D,
                                               int c, int g, typename Traits<T>::frag (&x)[CB][NK]) {
  // Every chunk is loaded, from a (row, column) clamped into the tensor, and dropped by a select where it lies past the head
  // size or the sequence: under `if (row < N && d < D)` each load sat in a block of its own and was waited for there — NK
  // dependent round trips per operand in front of the first K/V tile (ten at head size 160, thirty in the dQ kernel, which
  // loads Q, dO and O this way).
  if constexpr (sizeof(T) == 4 && NK > 5) {   // fp32 at head sizes > 80 (register budget; not a shape any UNet here runs)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int row = row0 + cb * 16 + c;
#pragma unroll
      for (int kc = 0; kc < NK; ++kc) {
        const int d = kc * 16 + 4 * g;
        x[cb][kc] = zero_frag<T>();
        if (row < N && d < D) x[cb][kc] = load_frag<T>(base + (size_t)row * row_stride + d);
      }
    }
    return;
  }
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int row = row0 + cb * 16 + c;
    const T* src = base + (size_t)min(row, N - 1) * row_stride;
    typename Traits<T>::frag v[NK];
#pragma unroll
    for (int kc = 0; kc < NK; ++kc) v[kc] = load_frag<T>(src + min(kc * 16 + 4 * g, D - 4));
#pragma unroll
    for (int kc = 0; kc < NK; ++kc) x[cb][kc] = (row < N && kc * 16 + 4 * g < D) ? v[kc] : zero_frag<T>();
  }
}

// out^T accumulators [NK][CB] (feature rows, this lane's column) -> global rows [col][d], scaled per column block
// x *= f, rounded once to T (the softmax scale folded into the Q operand: the MFMA then delivers log2-domain scores)
template <typename T, int NK, int CB>
__device__ __forceinline__ void scale_frags(typename Traits<T>::frag (&x)[CB][NK], float f) {
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int kc = 0; kc < NK; ++kc)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[cb][kc][r] = Traits<T>::from_f32(Traits<T>::to_f32(x[cb][kc][r]) * f);
}

template <typename T, int NK, int CB>
__device__ __forceinline__ void store_colsT(T* __restrict__ base, size_t row_stride, int row0, int N, int D, int c,
                                            int g, const f32x4 (&acc)[NK][CB], const float (&mul)[CB]) {
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int row = row0 + cb * 16 + c;
    if (row >= N) continue;
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) {
      const int d = dt * 16 + 4 * g;
      if (d < D) {
        typename Traits<T>::frag o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = Traits<T>::from_f32(acc[dt][cb][r] * mul[cb]);
        store_frag<T>(base + (size_t)row * row_stride + d, o);
      }
    }
  }
}

// Workgroup -> (batch, head, tile).  Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8), each with its
// own L2; every tile of one (batch, head) pair sweeps that pair's whole K / V (or Q / dO), so a pair's tiles should
// share an XCD.  The launch index is therefore re-read as "XCD-major": XCD x takes the contiguous range
// [x * W/8, (x+1) * W/8) of the pair-major work list (the W % 8 leftovers keep their place at the end).  With 8 heads
// at batch 1 this is the old head-fastest order (one head per XCD); with 5 / 10 / 20 heads (SD-2.x, SDXL) it replaces
// an order that smeared every head over all eight L2s (PMC: 9x the algorithmic bytes fetched past L2).  Placement is a
// speed matter only: nothing depends on which XCD a workgroup really lands on.
__device__ __forceinline__ void decode_block(int H, int ntile, int& b, int& head, int& tile) {
  const unsigned W = gridDim.x, bid = blockIdx.x, cpx = W >> 3;
  const unsigned j = bid < (cpx << 3) ? (bid & 7u) * cpx + (bid >> 3) : bid;
  const unsigned pair = j / (unsigned)ntile;
  tile = (int)(j - pair * (unsigned)ntile);
  head = (int)(pair % (unsigned)H);
  b = (int)(pair / (unsigned)H);
}

// raw v_exp_f32: arguments here are <= 0 (or the result is multiplied by something that dominates), so the
// denormal-range fix-up sequence of exp2f (compare / select / ldexp per element) is dead weight
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float quad_max(float v) {  // over the 4 lanes (g = 0..3) that share a column
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// Power-of-two running scale for accumulator tiles that enter a 16-bit MFMA as operands (dS): values are kept
// <= 1 in magnitude relative to the largest seen so far; returns the exponent to apply now and rescales `acc`
// (exact) when a larger magnitude arrives.  E is the current exponent (acc holds true * 2^E).
template <int NK, int CB>
__device__ __forceinline__ void rescale_running(float amax, int cb, int& E, f32x4 (&acc)[NK][CB]) {
  if (!(amax > 0.f) || amax == INFINITY) return;
  int e;
  (void)frexpf(amax, &e);  // amax = m * 2^e, m in [0.5, 1)
  const int want = -e < -120 ? -120 : (-e > 99 ? 99 : -e);  // keeps 2^E and 2^-E finite f32 (scale_of)
  if (want < E) {
    const float f = ldexpf(1.0f, want - E);
#pragma unroll
    for (int dt = 0; dt < NK; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[dt][cb][r] *= f;
    E = want;
  }
}

constexpr int kNoExp = 100;  // "no data yet" exponent (2^100 * 0 = 0)
constexpr float kGrow = 16.0f;  // backward: |dS| * 2^E may reach this before the scale is renewed (fp16 max 65504)
__device__ __forceinline__ float scale_of(int E) { return __uint_as_float((unsigned)(127 + E) << 23); }  // 2^E
constexpr float kLazy = 8.0f;  // forward: the running maximum is only raised when a score tops it by > 2^kLazy

// =================================================================================================== forward
// Softmax on a diet (the loop is VALU-issue bound at head_dim 40: 3.5 MFMAs per 16x16 score block against the vector
// instructions of 4 scores per lane):
//   * Q is pre-multiplied by scale * log2(e) once, so the MFMA delivers log2-domain scores;
//   * the running maximum enters as the C operand of each score chain (C = -m): the accumulators come out as s - m,
//     ready for v_exp_f32 — no subtract, no zeroing of the accumulators;
//   * ONES (head sizes that are not a multiple of 16, e.g. 40): the first pad column of the V image holds 1.0, so the
//     P.V product itself accumulates the row sum (of the same rounded P that multiplies V) in output row D;
//   * what is left per score: v_exp_f32, half a v_cvt_pk, half a v_max3 (the lazy-maximum test).
// Lazy maximum: m only moves when a score would exceed it by more than 2^kLazy (wave ballot; forced on the first
// tile, where m starts at 0); then O, the sums and this tile's scores are rescaled by the same factor.
template <typename T, int NK, int QB, int NBUF, int KT, bool ONES, int NW>
__global__ __launch_bounds__(64 * NW) void self_attn_fwd_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                                 const T* __restrict__ V, T* __restrict__ O,
                                                                 float* __restrict__ LSE, int H, int N, int D, int nqt,
                                                                 int ldq, float scale) {
  using Tr = Traits<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // one buffer = [K row-major | V column image]; buffers are addressed as base + cur * kBuf so that the compiler
  // keeps the LDS address space (a local array of pointers decays to generic pointers -> flat_load + vmcnt(0))
  constexpr int kOne = row_img<T, NK, KT>() + col_img<T, NK, KT>();
  constexpr int kBuf = NBUF == 2 ? kOne : 0;
  constexpr int kVoff = row_img<T, NK, KT>();
  T* const lds = reinterpret_cast<T*>(smem);

  int b, head, qt;
  decode_block(H, nqt, b, head, qt);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const size_t rs = (size_t)ldq;     // row stride of Q / K / V (H*D, or 3*H*D when they are slices of a fused QKV)
  const size_t rso = (size_t)H * D;  // row stride of O
  const T* Qb = Q + (size_t)b * N * rs + (size_t)head * D;
  const T* Kb = K + (size_t)b * N * rs + (size_t)head * D;
  const T* Vb = V + (size_t)b * N * rs + (size_t)head * D;
  const int q0 = qt * (NW * QB * 16) + wave * (QB * 16);
  const int ones_d = ONES ? D : -1;

  typename Tr::frag qf[QB][NK];
  load_col_frags<T, NK, QB>(Qb, rs, q0, N, D, c, g, qf);
  scale_frags<T, NK, QB>(qf, scale * 1.4426950408889634f);

  const int ntiles = (N + KT - 1) / KT;
  Stage<T, NK, KT, true, 64 * NW> sk, sv;
  sk.init(Kb, D, rs);
  sv.init(Vb, D, rs);
  sk.load(0, N, rs);
  sv.load(0, N, rs);
  sk.store(lds, nullptr);
  store_tile(sv, (T*)nullptr, lds + kVoff, ones_d);
  __syncthreads();

  f32x4 o[NK][QB], negm[QB];
  float m[QB], l[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    m[qb] = 0.f;
    l[qb] = 0.f;
    negm[qb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) o[dt][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // Everything loaded so far (the Q fragments) has landed by now; say so.  Without this the compiler cannot prove it
  // on every path into the loop and parks an s_waitcnt vmcnt(0) in front of the tile's first MFMA — which in steady
  // state waits for the NEXT tile's prefetch, issued a few instructions earlier.
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt / lgkmcnt untouched
  // Staging order with two LDS buffers: the registers always hold tile kt + 1 (loaded during tile kt - 1's math); at
  // the top of iteration kt they go to the other buffer — free since the barrier that ended iteration kt - 1 — and
  // the loads of tile kt + 2 are issued at once.  The LDS writes then overlap the tile's math instead of sitting
  // between the math and the barrier, where every wave waits for the slowest writer.
  if (NBUF == 2 && ntiles > 1) {
    sk.load(KT, N, rs);
    sv.load(KT, N, rs);
  }
  for (int kt = 0; kt < ntiles; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < ntiles;
    if (NBUF == 2) {
      if (more) {
        T* nxt = lds + (cur ^ 1) * kBuf;
        sk.store(nxt, nullptr);
        store_tile(sv, (T*)nullptr, nxt + kVoff, ones_d);
        if (kt + 2 < ntiles) {
          sk.load((kt + 2) * KT, N, rs);
          sv.load((kt + 2) * KT, N, rs);
        }
      }
    } else if (more) {  // single buffer: prefetch to registers now, write after this tile's math and a barrier
      sk.load((kt + 1) * KT, N, rs);
      sv.load((kt + 1) * KT, N, rs);
    }
    {  // the tile's scores and probabilities live in registers inside this scope only
      f32x4 s[KT / 16][QB];
      const T* kimg = lds + cur * kBuf;
      const T* vimg = kimg + kVoff;
      // 16 queries per wave leave the registers for whole-tile read-ahead (K before the score MFMAs, V under the
      // softmax); the 32-query variant keeps the depth-2 pipelines
      constexpr bool kAhead = kTrRead<T> && ((QB == 1 && NK <= 5) || (QB == 2 && NK <= 3));
      rows_times_cols<T, NK, KT / 16, QB, kAhead ? KT / 16 : 1, true>(kimg, qf, c, g, s, negm);  // s = q.k - m
      ColFrags<T, NK, kAhead ? KT / 16 : 2> vfr;
      if constexpr (kAhead) vfr.load(vimg, lane);
      const int key0 = kt * KT;
      if (key0 + KT > N) {  // only the last, partial tile needs the key mask (uniform branch)
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
          for (int kb = 0; kb < KT / 16; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (key0 + kb * 16 + 4 * g + r >= N) s[kb][qb][r] = -INFINITY;
      }
      float tmax[QB];
      bool grow = kt == 0;
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        // four independent chains (one per accumulator element), joined at the end: a single running maximum is a
        // dependent chain of KT/8 v_max3 — serial latency the wave cannot hide at two waves per SIMD
        float m4[4] = {s[0][qb][0], s[0][qb][1], s[0][qb][2], s[0][qb][3]};
#pragma unroll
        for (int kb = 1; kb + 1 < KT / 16; kb += 2)
#pragma unroll
          for (int r = 0; r < 4; ++r) m4[r] = fmaxf(fmaxf(m4[r], s[kb][qb][r]), s[kb + 1][qb][r]);
        if constexpr ((KT / 16) % 2 == 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) m4[r] = fmaxf(m4[r], s[KT / 16 - 1][qb][r]);
        }
        tmax[qb] = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
        grow |= tmax[qb] > kLazy;
      }
      if (__builtin_amdgcn_ballot_w64(grow) != 0) {  // wave-uniform; typically the first tile or two only
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
          float d = quad_max(tmax[qb]);      // by how much this column's maximum moves (the first tile: from 0, any sign)
          if (kt != 0) d = fmaxf(d, 0.f);
          const float alpha = kt != 0 ? fast_exp2(-d) : 1.0f;
          m[qb] += d;
          l[qb] *= alpha;
          negm[qb] = f32x4{-m[qb], -m[qb], -m[qb], -m[qb]};
#pragma unroll
          for (int dt = 0; dt < NK; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][qb][r] *= alpha;
#pragma unroll
          for (int kb = 0; kb < KT / 16; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kb][qb][r] -= d;
        }
      }
      typename Tr::frag pf[KT / 16][QB];
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        float sum = 0.f;
#pragma unroll
        for (int kb = 0; kb < KT / 16; ++kb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pr = fast_exp2(s[kb][qb][r]);
            if (!ONES) sum += pr;
            pf[kb][qb][r] = Tr::from_f32(pr);
          }
        }
        if (!ONES) l[qb] += sum;  // this lane's share of the row sum
      }
      if constexpr (kAhead) vfr.template apply<QB>(pf, o);
      else tileT_times_frags<T, NK, KT / 16, QB>(vimg, pf, lane, o);
    }
    if (NBUF == 1) {
      __syncthreads();  // single buffer: everyone is done reading before it is overwritten
      if (more) {
        sk.store(lds, nullptr);
        store_tile(sv, (T*)nullptr, lds + kVoff, ones_d);
      }
    }
    __syncthreads();
  }
  float inv[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    // ONES: output row D of O^T (feature block NK - 1, row D % 16 = 8 -> lanes g = 2, element 0) holds the row sum
    const float lsum = ONES ? __shfl(o[NK - 1][qb][0], c + 32, 64) : quad_sum(l[qb]);
    inv[qb] = 1.0f / lsum;
    const int q = q0 + qb * 16 + c;
    if (LSE != nullptr && g == 0 && q < N) LSE[((size_t)b * H + head) * N + q] = m[qb] + log2f(lsum);
  }
  store_colsT<T, NK, QB>(O + ((size_t)b * N * H + head) * D, rso, q0, N, D, c, g, o, inv);
}

// =================================================================================================== cotangent on P
// A cotangent dP on the probabilities themselves (a loss that reads the stored self-attention maps) turns the score gradient
// into dS = P o (dO V^T + dP - delta - r), r[n] = sum_k P[n][k] dP[n][k]: one more additive tile in the dP chain and one more
// row constant.  The HAS_DP instantiations of the two backward bodies below add them; r comes from a row pre-pass
// (self_attn_rowdot_kernel).  The map of (b, h) starts at dP + (b H + h) * dp_stride (0: one map shared by every head-map),
// rows dense.  The tile goes straight from global memory to the registers of the lane that owns the score — in the dQ kernel
// and the pre-pass a lane owns four consecutive keys of one query (one 8-byte load in the 16-bit types when vec_ok: dP
// aligned to four elements, N % 4 == 0, dp_stride % 4 == 0; four element loads otherwise), in the dK/dV kernel four
// consecutive queries of one key (four element loads).  Every address is clamped into the map and the whole tile is
// requested in one batch in front of the tile's MFMA chains; dead rows and columns are dropped where the value is consumed.
template <typename T>
__device__ __forceinline__ typename Traits<T>::frag load_dp_run(const T* __restrict__ row, int key, int N, bool vec_ok) {
  if (vec_ok) return load_frag<T>(row + min(key, N - 4));   // N % 4 == 0: a run is all in or all out
  typename Traits<T>::frag f;
#pragma unroll
  for (int r = 0; r < 4; ++r) f[r] = row[min(key + r, N - 1)];
  return f;
}

// =================================================================================================== backward dQ
// HAS_DP (self_attn_bwd_dp_dq_kernel): dP / dp_stride / vec_ok / rowdot as above; dO and O may then both be null (= zeros).
template <typename T, int NK, int QB, int NBUF, int KT, bool HAS_DP>
__device__ __forceinline__ void bwd_dq_body(const T* Q, const T* K, const T* V,
                                            const T* O, const T* dO, const T* dP,
                                            size_t dp_stride, bool vec_ok, const float* LSE,
                                            float* delta, const float* rowdot,
                                            T* dQ, int H, int N, int D, int nqt, int ldq, float scale) {
  using Tr = Traits<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // one buffer = [K row-major | V row-major | K column image (transposed, or row-major for the transposing read)]
  T* const lds = reinterpret_cast<T*>(smem);
  constexpr int kVoff = row_img<T, NK, KT>(), kToff = 2 * row_img<T, NK, KT>();
  constexpr int kBuf = NBUF == 2 ? 2 * row_img<T, NK, KT>() + col_img<T, NK, KT>() : 0;
  int b, head, qt;
  decode_block(H, nqt, b, head, qt);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const size_t rs = (size_t)ldq, rso = (size_t)H * D;
  const size_t off = (size_t)b * N * rs + (size_t)head * D;    // into Q / K / V / dQ
  const size_t offo = ((size_t)b * N * H + head) * D;          // into dO
  const int q0 = qt * (4 * QB * 16) + wave * (QB * 16);
  const float c1 = scale * 1.4426950408889634f;

  const bool has_do = !HAS_DP || dO != nullptr;   // wave-uniform
  const T* dPb = nullptr;                          // this (batch, head)'s map
  if constexpr (HAS_DP) dPb = dP + ((size_t)b * H + head) * dp_stride;
  typename Tr::frag qf[QB][NK], dof[QB][NK];
  load_col_frags<T, NK, QB>(Q + off, rs, q0, N, D, c, g, qf);
  if (has_do) {
    load_col_frags<T, NK, QB>(dO + offo, rso, q0, N, D, c, g, dof);
  } else {
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int kc = 0; kc < NK; ++kc) dof[qb][kc] = zero_frag<T>();
  }
  // delta[q] = sum_d dO[q][d] O[q][d]: this wave holds its queries' dO rows as fragments anyway; with the O rows
  // beside them the row sum is 12 FMAs and the column's cross-lane step — no separate pass over O and dO.  The
  // values also go to `delta` for the dK/dV kernel that follows on the stream.
  float lse[QB], dl[QB];
  {
    typename Tr::frag of[QB][NK];
    if (has_do) {
      load_col_frags<T, NK, QB>(O + offo, rso, q0, N, D, c, g, of);
    } else {
#pragma unroll
      for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int kc = 0; kc < NK; ++kc) of[qb][kc] = zero_frag<T>();
    }
    // (one straight-line sum with and without dO: the products contract into the same FMAs in every instantiation)
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      float part = 0.f;
#pragma unroll
      for (int kc = 0; kc < NK; ++kc)
#pragma unroll
        for (int r = 0; r < 4; ++r) part += Tr::to_f32(dof[qb][kc][r]) * Tr::to_f32(of[qb][kc][r]);
      dl[qb] = quad_sum(part);
      const int q = q0 + qb * 16 + c;
      lse[qb] = q < N ? LSE[((size_t)b * H + head) * N + q] : 0.f;
      if (g == 0 && q < N) delta[((size_t)b * H + head) * N + q] = dl[qb];
      if constexpr (HAS_DP) {   // the dP chain starts from -(delta + r)
        const float rd = rowdot[((size_t)b * H + head) * N + min(q, N - 1)];
        dl[qb] += q < N ? rd : 0.f;
      }
    }
  }
  scale_frags<T, NK, QB>(qf, c1);  // log2-domain scores straight out of the MFMA (as in the forward)
  // staging as in the forward (double buffer): the registers hold tile kt + 1 at the top of iteration kt, go to the
  // other LDS buffer there (under the tile's math, not between math and barrier) and are refilled with tile kt + 2
  constexpr bool kPre = NBUF == 2;
  Stage<T, NK, KT, kPre> sk, sv;
  sk.init(K + off, D, rs);
  sv.init(V + off, D, rs);
  sk.load(0, N, rs);
  sv.load(0, N, rs);
  store_tile(sk, lds, lds + kToff);
  sv.store(lds + kVoff, nullptr);
  __syncthreads();

  // Row constants as initial accumulators: the score chain starts from -LSE (+ E: the power-of-two scale of dS for
  // the 16-bit MFMA, so p * 2^E = exp2(s - LSE + E) costs nothing), the dP chain from -delta.  Per score that leaves
  // v_exp_f32, one multiply, half a v_max3 (|dS| against the renewal threshold) and half a v_cvt_pk.
  constexpr bool kScaled = sizeof(T) == 2;
  f32x4 acc[NK][QB], cs[QB], cdp[QB];
  int E[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    E[qb] = kScaled ? kNoExp : 0;
    const float c0 = (float)E[qb] - lse[qb];
    cs[qb] = f32x4{c0, c0, c0, c0};
    cdp[qb] = f32x4{-dl[qb], -dl[qb], -dl[qb], -dl[qb]};
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) acc[dt][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int ntiles = (N + KT - 1) / KT;
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): Q / dO / O fragments have landed (see the forward)
  if (NBUF == 2 && ntiles > 1) {
    sk.load(KT, N, rs);
    sv.load(KT, N, rs);
  }
  for (int kt = 0; kt < ntiles; ++kt) {
    const int cur = kt & 1;
    if (NBUF == 2) {
      if (kt + 1 < ntiles) {
        T* nxt = lds + (cur ^ 1) * kBuf;
        store_tile(sk, nxt, nxt + kToff);
        sv.store(nxt + kVoff, nullptr);
        if (kt + 2 < ntiles) {
          sk.load((kt + 2) * KT, N, rs);
          sv.load((kt + 2) * KT, N, rs);
        }
      }
    } else if (kt + 1 < ntiles) {
      sk.load((kt + 1) * KT, N, rs);
      sv.load((kt + 1) * KT, N, rs);
    }
    f32x4 s[KT / 16][QB], dp[KT / 16][QB];
    const T* buf = lds + cur * kBuf;
    const int key0 = kt * KT;
    typename Tr::frag dpf[HAS_DP ? KT / 16 : 1][QB];   // this lane's runs of the dP tile, in flight under the two chains
    if constexpr (HAS_DP) {
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        const T* row = dPb + (size_t)min(q0 + qb * 16 + c, N - 1) * (size_t)N;
#pragma unroll
        for (int kb = 0; kb < KT / 16; ++kb) dpf[kb][qb] = load_dp_run<T>(row, key0 + kb * 16 + 4 * g, N, vec_ok);
      }
    }
    // 16 columns per wave leave registers for whole-tile read-ahead (see the forward)
    constexpr bool kAhead = kTrRead<T> && QB == 1 && NK <= 5;
    constexpr int kA = kAhead ? KT / 16 : 1;
    rows_times_cols<T, NK, KT / 16, QB, kA, true>(buf, qf, c, g, s, cs);            // s  = q.k - LSE + E
    rows_times_cols<T, NK, KT / 16, QB, kA, true>(buf + kVoff, dof, c, g, dp, cdp);  // dp = dO.v - delta
    ColFrags<T, NK, kAhead ? KT / 16 : 2> kcol;
    if constexpr (kAhead) kcol.load(buf + kToff, lane);
    if constexpr (HAS_DP) {   // dp += dP tile, before |dS| 2^E is formed
      const bool edge = key0 + KT > N || q0 + QB * 16 > N;   // wave-uniform
#pragma unroll
      for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int kb = 0; kb < KT / 16; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float x = Tr::to_f32(dpf[kb][qb][r]);
            const bool live = !edge || (key0 + kb * 16 + 4 * g + r < N && q0 + qb * 16 + c < N);
            dp[kb][qb][r] += live ? x : 0.f;
          }
    }
    if (key0 + KT > N) {  // partial last tile: masked keys get p = exp2(-inf) = 0
#pragma unroll
      for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int kb = 0; kb < KT / 16; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (key0 + kb * 16 + 4 * g + r >= N) s[kb][qb][r] = -INFINITY;
    }
    float amax[QB];
    bool grow = false;
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      float am = 0.f;
#pragma unroll
      for (int kb = 0; kb < KT / 16; ++kb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kb][qb][r] = fast_exp2(s[kb][qb][r]) * dp[kb][qb][r];  // dS * 2^E
        am = fmaxf(fmaxf(am, fmaxf(fabsf(s[kb][qb][0]), fabsf(s[kb][qb][1]))), fmaxf(fabsf(s[kb][qb][2]), fabsf(s[kb][qb][3])));
      }
      amax[qb] = am;
      grow |= am > kGrow;
    }
    // lazy power-of-two scale (16-bit operands): only when some |dS| * 2^E outgrows 2^4 (always on the first tile,
    // where E starts at 2^100) does the wave reduce the column maxima across lanes and renew the scale
    if (kScaled && __builtin_amdgcn_ballot_w64(grow) != 0) {
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        const float am = quad_max(amax[qb]);
        if (am > 0.f && am < INFINITY) {
          int e;
          (void)frexpf(am, &e);  // am = mant * 2^e, mant in [0.5, 1): the new scale brings it back to [0.5, 1)
          int want = E[qb] - e;
          want = want < -120 ? -120 : (want > 99 ? 99 : want);
          if (want < E[qb]) {
            const float f = ldexpf(1.0f, want - E[qb]);
#pragma unroll
            for (int dt = 0; dt < NK; ++dt)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[dt][qb][r] *= f;
#pragma unroll
            for (int kb = 0; kb < KT / 16; ++kb)
#pragma unroll
              for (int r = 0; r < 4; ++r) s[kb][qb][r] *= f;
            E[qb] = want;
            const float c0 = (float)want - lse[qb];
            cs[qb] = f32x4{c0, c0, c0, c0};
          }
        }
      }
    }
    typename Tr::frag dsf[KT / 16][QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int kb = 0; kb < KT / 16; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) dsf[kb][qb][r] = Tr::from_f32(s[kb][qb][r]);
    if constexpr (kAhead) kcol.template apply<QB>(dsf, acc);
    else tileT_times_frags<T, NK, KT / 16, QB>(buf + kToff, dsf, lane, acc);
    if (NBUF == 1) {
      __syncthreads();
      if (kt + 1 < ntiles) {
        store_tile(sk, lds, lds + kToff);
        sv.store(lds + kVoff, nullptr);
      }
    }
    __syncthreads();
  }
  float mul[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) mul[qb] = (kScaled && E[qb] != kNoExp) ? scale * ldexpf(1.0f, -E[qb]) : scale;
  store_colsT<T, NK, QB>(dQ + off, rs, q0, N, D, c, g, acc, mul);
}

template <typename T, int NK, int QB, int NBUF, int KT>
__global__ __launch_bounds__(kThreads) void self_attn_bwd_dq_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                                    const T* __restrict__ V, const T* __restrict__ O,
                                                                    const T* __restrict__ dO,
                                                                    const float* __restrict__ LSE,
                                                                    float* __restrict__ delta, T* __restrict__ dQ,
                                                                    int H, int N, int D, int nqt, int ldq, float scale) {
  bwd_dq_body<T, NK, QB, NBUF, KT, false>(Q, K, V, O, dO, nullptr, 0, false, LSE, delta, nullptr, dQ, H, N, D, nqt, ldq, scale);
}

// (a name of its own: tools that pick kernels by a substring of self_attn_bwd_dq_kernel<...> keep meaning the plain one)
template <typename T, int NK, int QB, int NBUF, int KT>
__global__ __launch_bounds__(kThreads) void self_attn_bwd_dp_dq_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                                       const T* __restrict__ V, const T* __restrict__ O,
                                                                       const T* __restrict__ dO, const T* __restrict__ dP,
                                                                       size_t dp_stride, int vec_ok,
                                                                       const float* __restrict__ LSE,
                                                                       float* __restrict__ delta,
                                                                       const float* __restrict__ rowdot,
                                                                       T* __restrict__ dQ, int H, int N, int D, int nqt,
                                                                       int ldq, float scale) {
  bwd_dq_body<T, NK, QB, NBUF, KT, true>(Q, K, V, O, dO, dP, dp_stride, vec_ok != 0, LSE, delta, rowdot, dQ, H, N, D, nqt, ldq,
                                         scale);
}

// =================================================================================================== backward dK, dV
// A wave owns KB x 16 keys on its lanes; the workgroup sweeps 64-query tiles (Q and dO row-major + transposed images).
// HAS_DP (self_attn_bwd_dp_dkdv_kernel): the dP tile joins the dP chain, the row constant is -(delta + r); dO may be null.
template <typename T, int NK, int KB, int NBUF, int KT, bool HAS_DP>
__device__ __forceinline__ void bwd_dkdv_body(const T* Q, const T* K, const T* V,
                                              const T* dO, const T* dP, size_t dp_stride,
                                              const float* LSE, const float* delta,
                                              const float* rowdot, T* dK, T* dV,
                                              int H, int N, int D, int nkt, int ldq, float scale) {
  using Tr = Traits<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // one buffer = [Q row-major | Q column image | dO row-major | dO column image]; then the per-query LSE / delta rows
  T* const lds = reinterpret_cast<T*>(smem);
  constexpr int kQt = row_img<T, NK, KT>(), kDr = kQt + col_img<T, NK, KT>(), kDt = kDr + row_img<T, NK, KT>();
  constexpr int kOne = 2 * row_img<T, NK, KT>() + 2 * col_img<T, NK, KT>();
  constexpr int kBuf = NBUF == 2 ? kOne : 0;
  float* const stats = reinterpret_cast<float*>(lds + NBUF * kOne);  // [2][2][KT]: (LSE, delta) per buffer
  constexpr int kSbuf = 2 * KT;
  int b, head, ktile;
  decode_block(H, nkt, b, head, ktile);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const size_t rs = (size_t)ldq, rso = (size_t)H * D;
  const size_t off = (size_t)b * N * rs + (size_t)head * D;    // into Q / K / V / dK / dV
  const size_t offo = ((size_t)b * N * H + head) * D;          // into dO
  const size_t soff = ((size_t)b * H + head) * N;
  const int k0 = ktile * (4 * KB * 16) + wave * (KB * 16);
  const float c1 = scale * 1.4426950408889634f;

  typename Tr::frag kf[KB][NK], vf[KB][NK];
  load_col_frags<T, NK, KB>(K + off, rs, k0, N, D, c, g, kf);
  load_col_frags<T, NK, KB>(V + off, rs, k0, N, D, c, g, vf);

  constexpr bool kPre = NBUF == 2;
  Stage<T, NK, KT, kPre> sq, sd;
  float pl = 0.f, pd = 0.f;  // this thread's prefetched -LSE / -delta entry (threads 0..63)
  auto load_stats = [&](int q0t) {
    if (threadIdx.x < KT) {
      const int q = q0t + threadIdx.x;
      pl = q < N ? -LSE[soff + q] : 0.f;
      pd = q < N ? -delta[soff + q] : 0.f;
      if constexpr (HAS_DP) pd -= q < N ? rowdot[soff + q] : 0.f;
    }
  };
  const bool has_do = !HAS_DP || dO != nullptr;   // wave-uniform; without dO its tiles are zeros and nothing is loaded
  const T* dPb = nullptr;
  if constexpr (HAS_DP) dPb = dP + ((size_t)b * H + head) * dp_stride;
  auto load_do = [&](int row0) {
    if (has_do) {
      sd.load(row0, N, rso);
    } else {
      sd.tile_row0 = 0;
      sd.seq_rows = N;
#pragma unroll
      for (int u = 0; u < decltype(sd)::PER; ++u) sd.v[u] = uint4{0, 0, 0, 0};
    }
  };
  sq.init(Q + off, D, rs);
  // The Q tile's row image feeds the score chain and holds Q' = round_T(c1 Q), the very operand the forward and the dQ kernel
  // make in registers: exp2(Q'.K - LSE) is then the forward's own probability, rows summing to 1.  (Scaling this wave's K
  // fragments instead is free, but perturbs every score by |s| u_T against the LSE of the forward's scores: on peaked rows in
  // bf16 the probability that should be 1 came out up to 20 % off, and dK / dV with it.)  The column image that feeds
  // dK = dS^T Q stays unscaled.
  auto store_q = [&](T* row_image, T* col_image) {
    store_tile(sq, (T*)nullptr, col_image);   // first: the staged registers are dead once the scaled copy is made from them
    sq.store_scaled(row_image, c1);
  };
  sd.init(has_do ? dO + offo : nullptr, D, rso);
  sq.load(0, N, rs);
  load_do(0);
  load_stats(0);
  store_q(lds, lds + kQt);
  store_tile(sd, lds + kDr, lds + kDt);
  if (threadIdx.x < KT) {
    stats[threadIdx.x] = pl;
    stats[KT + threadIdx.x] = pd;
  }
  __syncthreads();

  constexpr bool kScaled = sizeof(T) == 2;
  f32x4 dk[NK][KB], dv[NK][KB];
  int E[KB];
  float fE[KB];  // 2^E
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    E[kb] = kScaled ? kNoExp : 0;
    fE[kb] = kScaled ? scale_of(kNoExp) : 1.0f;
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) dk[dt][kb] = dv[dt][kb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int ntiles = (N + KT - 1) / KT;
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the K / V fragments have landed
  if (NBUF == 2 && ntiles > 1) {
    sq.load(KT, N, rs);
    load_do(KT);
    load_stats(KT);
  }
  for (int qt = 0; qt < ntiles; ++qt) {
    const int cur = qt & 1;
    if (NBUF == 2) {
      if (qt + 1 < ntiles) {   // registers -> the other buffer (free since the last barrier), then refill them
        T* nxt = lds + (cur ^ 1) * kBuf;
        store_q(nxt, nxt + kQt);
        store_tile(sd, nxt + kDr, nxt + kDt);
        if (threadIdx.x < KT) {
          stats[(cur ^ 1) * kSbuf + threadIdx.x] = pl;
          stats[(cur ^ 1) * kSbuf + KT + threadIdx.x] = pd;
        }
        if (qt + 2 < ntiles) {
          sq.load((qt + 2) * KT, N, rs);
          load_do((qt + 2) * KT);
          load_stats((qt + 2) * KT);
        }
      }
    } else if (qt + 1 < ntiles) {
      sq.load((qt + 1) * KT, N, rs);
      load_do((qt + 1) * KT);
      load_stats((qt + 1) * KT);
    }
    // S[q rows][key cols] and dP[q rows][key cols]; the query rows' -LSE / -delta (f32x4 per row block, straight from
    // LDS) are the initial accumulators of the two chains
    f32x4 s[KT / 16][KB], dp[KT / 16][KB];
    const T* buf = lds + cur * kBuf;
    const int q0t = qt * KT;
    typename Tr::frag dpf[HAS_DP ? KT / 16 : 1][KB];   // dP[four queries of a row block][this lane's key], in flight under the chains
    if constexpr (HAS_DP) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const T* col = dPb + min(k0 + kb * 16 + c, N - 1);
#pragma unroll
        for (int qb = 0; qb < KT / 16; ++qb)
#pragma unroll
          for (int r = 0; r < 4; ++r) dpf[qb][kb][r] = col[(size_t)min(q0t + qb * 16 + 4 * g + r, N - 1) * (size_t)N];
      }
    }
    const float* Lq = stats + cur * kSbuf;
    const float* Dq = Lq + KT;
    f32x4 cl[KT / 16], cd[KT / 16];
#pragma unroll
    for (int qb = 0; qb < KT / 16; ++qb) {
      cl[qb] = *reinterpret_cast<const f32x4*>(Lq + qb * 16 + 4 * g);
      cd[qb] = *reinterpret_cast<const f32x4*>(Dq + qb * 16 + 4 * g);
    }
    constexpr bool kAhead = kTrRead<T> && KB == 1 && NK <= 5;
    constexpr int kA = kAhead ? KT / 16 : 1;
    rows_times_cols<T, NK, KT / 16, KB, kA, true, true>(buf, kf, c, g, s, nullptr, cl);         // s  = q.k - LSE
    rows_times_cols<T, NK, KT / 16, KB, kA, true, true>(buf + kDr, vf, c, g, dp, nullptr, cd);  // dp = dO.v - delta
    ColFrags<T, NK, kAhead ? KT / 16 : 2> docol, qcol;
    if constexpr (kAhead) {
      docol.load(buf + kDt, lane);
      qcol.load(buf + kQt, lane);
    }
    typename Tr::frag pf[KT / 16][KB], dsf[KT / 16][KB];
    // wave-uniform: only the last query tile has dead rows, only the last key block of a ragged sequence dead columns
    const bool edge = q0t + KT > N || k0 + KB * 16 > N;
    if constexpr (HAS_DP) {   // dp += dP tile, before |dS| 2^E is formed
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int qb = 0; qb < KT / 16; ++qb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float x = Tr::to_f32(dpf[qb][kb][r]);
            const bool live = !edge || (k0 + kb * 16 + c < N && q0t + qb * 16 + 4 * g + r < N);
            dp[qb][kb][r] += live ? x : 0.f;
          }
    }
    if (edge) {  // dead rows / columns contribute nothing: p = exp2(-inf) = 0
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const bool key_live = k0 + kb * 16 + c < N;
#pragma unroll
        for (int qb = 0; qb < KT / 16; ++qb)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (!key_live || q0t + qb * 16 + 4 * g + r >= N) s[qb][kb][r] = -INFINITY;
      }
    }
    float amax[KB];
    bool grow = false;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      float am = 0.f;
#pragma unroll
      for (int qb = 0; qb < KT / 16; ++qb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = fast_exp2(s[qb][kb][r]);
          pf[qb][kb][r] = Tr::from_f32(pr);
          s[qb][kb][r] = (pr * fE[kb]) * dp[qb][kb][r];  // dS * 2^E
        }
        am = fmaxf(fmaxf(am, fmaxf(fabsf(s[qb][kb][0]), fabsf(s[qb][kb][1]))), fmaxf(fabsf(s[qb][kb][2]), fabsf(s[qb][kb][3])));
      }
      amax[kb] = am;
      grow |= am > kGrow;
    }
    if (kScaled && __builtin_amdgcn_ballot_w64(grow) != 0) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const float am = quad_max(amax[kb]);
        if (am > 0.f && am < INFINITY) {
          int e;
          (void)frexpf(am, &e);
          int want = E[kb] - e;
          want = want < -120 ? -120 : (want > 99 ? 99 : want);
          if (want < E[kb]) {
            const float f = ldexpf(1.0f, want - E[kb]);
#pragma unroll
            for (int dt = 0; dt < NK; ++dt)
#pragma unroll
              for (int r = 0; r < 4; ++r) dk[dt][kb][r] *= f;
#pragma unroll
            for (int qb = 0; qb < KT / 16; ++qb)
#pragma unroll
              for (int r = 0; r < 4; ++r) s[qb][kb][r] *= f;
            E[kb] = want;
            fE[kb] = scale_of(want);
          }
        }
      }
    }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int qb = 0; qb < KT / 16; ++qb)
#pragma unroll
        for (int r = 0; r < 4; ++r) dsf[qb][kb][r] = Tr::from_f32(s[qb][kb][r]);
    if constexpr (kAhead) {
      docol.template apply<KB>(pf, dv);   // dV^T += dO^T P
      qcol.template apply<KB>(dsf, dk);   // dK^T += Q^T dS
    } else {
      tileT_times_frags<T, NK, KT / 16, KB>(buf + kDt, pf, lane, dv);
      tileT_times_frags<T, NK, KT / 16, KB>(buf + kQt, dsf, lane, dk);
    }
    if (NBUF == 1) {
      __syncthreads();
      if (qt + 1 < ntiles) {
        store_q(lds, lds + kQt);
        store_tile(sd, lds + kDr, lds + kDt);
        if (threadIdx.x < KT) {   // the row statistics are double-buffered in both modes
          stats[(cur ^ 1) * kSbuf + threadIdx.x] = pl;
          stats[(cur ^ 1) * kSbuf + KT + threadIdx.x] = pd;
        }
      }
    }
    __syncthreads();
  }
  float mk[KB], one[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    // dK = scale * sum dS^T Q; the scores used the round_T(c1 Q) row image, the product here the unscaled column image:
    // only `scale` is left
    mk[kb] = (kScaled && E[kb] != kNoExp) ? scale * ldexpf(1.0f, -E[kb]) : scale;
    one[kb] = 1.0f;
  }
  store_colsT<T, NK, KB>(dK + off, rs, k0, N, D, c, g, dk, mk);
  store_colsT<T, NK, KB>(dV + off, rs, k0, N, D, c, g, dv, one);
}

template <typename T, int NK, int KB, int NBUF, int KT>
__global__ __launch_bounds__(kThreads) void self_attn_bwd_dkdv_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                                      const T* __restrict__ V,
                                                                      const T* __restrict__ dO,
                                                                      const float* __restrict__ LSE,
                                                                      const float* __restrict__ delta,
                                                                      T* __restrict__ dK, T* __restrict__ dV, int H,
                                                                      int N, int D, int nkt, int ldq, float scale) {
  bwd_dkdv_body<T, NK, KB, NBUF, KT, false>(Q, K, V, dO, nullptr, 0, LSE, delta, nullptr, dK, dV, H, N, D, nkt, ldq, scale);
}

template <typename T, int NK, int KB, int NBUF, int KT>
__global__ __launch_bounds__(kThreads) void self_attn_bwd_dp_dkdv_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                                         const T* __restrict__ V,
                                                                         const T* __restrict__ dO,
                                                                         const T* __restrict__ dP, size_t dp_stride,
                                                                         const float* __restrict__ LSE,
                                                                         const float* __restrict__ delta,
                                                                         const float* __restrict__ rowdot,
                                                                         T* __restrict__ dK, T* __restrict__ dV, int H,
                                                                         int N, int D, int nkt, int ldq, float scale) {
  bwd_dkdv_body<T, NK, KB, NBUF, KT, true>(Q, K, V, dO, dP, dp_stride, LSE, delta, rowdot, dK, dV, H, N, D, nkt, ldq, scale);
}

// =================================================================================================== probabilities
// P = softmax(scale Q K^T) written out, for a controller that keeps self-attention maps (reference capture mode).  The row
// statistic is known (the LSE the forward left), so there is no running maximum and no rescale: the score chain starts
// from -LSE (as in the dQ kernel), one v_exp_f32 per score, and the tile leaves.  Operands, rounding of the pre-scaled Q,
// MFMA instruction and k-chunk order are the forward's, so a stored row is the one the forward summed.  A wave owns 16
// queries on its lanes and sweeps 64-key tiles of K (row-major image, double-buffered, tile kt + 2 in flight in registers).
// Traffic per head: N * N elements of P out against 2 N D of operands in — store-bound; the stores therefore go through
// a per-wave LDS tile [16 queries][64 keys] and leave as 16-byte pieces, eight (f32: sixteen) lanes to a row.  That needs
// every row of P to start 16-byte aligned (vec_ok: P aligned and N * sizeof(T) % 16 == 0); otherwise each lane writes its
// sixteen probabilities one by one from the registers — the same values.  All offsets into P are 64-bit.
template <typename T, int NK>
__global__ __launch_bounds__(kThreads) void self_attn_probs_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                                    const float* __restrict__ LSE, T* __restrict__ P,
                                                                    int H, int N, int D, int nqt, int ldq, float scale,
                                                                    int vec_ok) {
  using Tr = Traits<T>;
  constexpr int KT = 64, NRB = KT / 16;
  constexpr int VEC = TL<T, KT>::VEC;
  constexpr int kKimg = row_img<T, NK, KT>();
  constexpr int SS = KT + VEC;             // row stride of the staging tile (16-byte aligned rows)
  constexpr int VPR = KT / VEC;            // 16-byte pieces per staged row
  constexpr int PER = 16 * VPR / 64;       // pieces per lane
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* const lds = reinterpret_cast<T*>(smem);   // [2][kKimg] K images, then [4 waves][16][SS] staging tiles

  int b, head, qt;
  decode_block(H, nqt, b, head, qt);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const size_t rs = (size_t)ldq;
  const size_t off = (size_t)b * N * rs + (size_t)head * D;   // into Q / K
  const size_t pair = (size_t)b * H + head;
  const int q0 = qt * (4 * 16) + wave * 16;
  const int q = q0 + c;
  T* const stage = lds + 2 * kKimg + wave * (16 * SS);
  T* const Pb = P + pair * (size_t)N * (size_t)N;

  typename Tr::frag qf[1][NK];
  load_col_frags<T, NK, 1>(Q + off, rs, q0, N, D, c, g, qf);
  const float lse_c = LSE[pair * N + min(q, N - 1)];   // clamped address, select below
  Stage<T, NK, KT, false> sk;
  sk.init(K + off, D, rs);
  sk.load(0, N, rs);
  scale_frags<T, NK, 1>(qf, scale * 1.4426950408889634f);
  const float nl = q < N ? -lse_c : 0.f;
  const f32x4 cs[1] = {f32x4{nl, nl, nl, nl}};
  sk.store(lds, nullptr);
  const int ntiles = (N + KT - 1) / KT;
  if (ntiles > 1) sk.load(KT, N, rs);
  __syncthreads();

  for (int kt = 0; kt < ntiles; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < ntiles) {   // registers -> the other buffer (free since the barrier that ended iteration kt - 1)
      sk.store(lds + (cur ^ 1) * kKimg, nullptr);
      if (kt + 2 < ntiles) sk.load((kt + 2) * KT, N, rs);
    }
    f32x4 s[NRB][1];
    constexpr bool kAhead = kTrRead<T> && NK <= 5;
    rows_times_cols<T, NK, NRB, 1, kAhead ? NRB : 1, true>(lds + cur * kKimg, qf, c, g, s, cs);   // s = q.k - LSE
    typename Tr::frag pf[NRB];
#pragma unroll
    for (int kb = 0; kb < NRB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) pf[kb][r] = Tr::from_f32(fast_exp2(s[kb][0][r]));
    const int key0 = kt * KT;
    if (vec_ok) {
#pragma unroll
      for (int kb = 0; kb < NRB; ++kb) store_frag<T>(stage + c * SS + kb * 16 + 4 * g, pf[kb]);
      // the tile is this wave's own: LDS serves a wave's accesses in order, the compiler only has to keep them so
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      uint4 piece[PER];
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int idx = u * 64 + lane;
        piece[u] = *reinterpret_cast<const uint4*>(stage + (idx / VPR) * SS + (idx % VPR) * VEC);
      }
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int idx = u * 64 + lane;
        const int row = q0 + idx / VPR, key = key0 + (idx % VPR) * VEC;   // N % VEC == 0: a piece is all in or all out
        if (row < N && key < N) *reinterpret_cast<uint4*>(Pb + (size_t)row * (size_t)N + key) = piece[u];
      }
    } else if (q < N) {
      T* const prow = Pb + (size_t)q * (size_t)N;
#pragma unroll
      for (int kb = 0; kb < NRB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = key0 + kb * 16 + 4 * g + r;
          if (key < N) prow[key] = pf[kb][r];
        }
    }
    __syncthreads();   // K buffer `cur` and the staging tiles are free again
  }
}

// =================================================================================================== row pre-pass for a cotangent on P
// r[n] = sum_k P[n][k] dP[n][k] per (batch, head): the probabilities kernel's sweep (same operands, same chain, P in f32 from
// the LSE) with a dot against the dP tile in place of the store.  The dot is this lane's sixteen products per tile in a fixed
// order, then the two cross-lane steps of the column: no atomics, the same bits every run.
template <typename T, int NK>
__global__ __launch_bounds__(kThreads) void self_attn_rowdot_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                                     const T* __restrict__ dP, size_t dp_stride, int vec_ok,
                                                                     const float* __restrict__ LSE,
                                                                     float* __restrict__ rowdot, int H, int N, int D,
                                                                     int nqt, int ldq, float scale) {
  using Tr = Traits<T>;
  constexpr int KT = 64, NRB = KT / 16;
  constexpr int kKimg = row_img<T, NK, KT>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* const lds = reinterpret_cast<T*>(smem);   // [2][kKimg] K images

  int b, head, qt;
  decode_block(H, nqt, b, head, qt);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const size_t rs = (size_t)ldq;
  const size_t off = (size_t)b * N * rs + (size_t)head * D;   // into Q / K
  const size_t pair = (size_t)b * H + head;
  const int q0 = qt * (4 * 16) + wave * 16;
  const int q = q0 + c;
  const T* const row = dP + pair * dp_stride + (size_t)min(q, N - 1) * (size_t)N;
  const bool vec = vec_ok != 0;

  typename Tr::frag qf[1][NK];
  load_col_frags<T, NK, 1>(Q + off, rs, q0, N, D, c, g, qf);
  const float lse_c = LSE[pair * N + min(q, N - 1)];   // clamped address, select below
  Stage<T, NK, KT, false> sk;
  sk.init(K + off, D, rs);
  sk.load(0, N, rs);
  scale_frags<T, NK, 1>(qf, scale * 1.4426950408889634f);
  const float nl = q < N ? -lse_c : 0.f;
  const f32x4 cs[1] = {f32x4{nl, nl, nl, nl}};
  sk.store(lds, nullptr);
  const int ntiles = (N + KT - 1) / KT;
  if (ntiles > 1) sk.load(KT, N, rs);
  __syncthreads();

  float part = 0.f;
  for (int kt = 0; kt < ntiles; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < ntiles) {   // registers -> the other buffer (free since the barrier that ended iteration kt - 1)
      sk.store(lds + (cur ^ 1) * kKimg, nullptr);
      if (kt + 2 < ntiles) sk.load((kt + 2) * KT, N, rs);
    }
    const int key0 = kt * KT;
    typename Tr::frag dpf[NRB];
#pragma unroll
    for (int kb = 0; kb < NRB; ++kb) dpf[kb] = load_dp_run<T>(row, key0 + kb * 16 + 4 * g, N, vec);
    f32x4 s[NRB][1];
    constexpr bool kAhead = kTrRead<T> && NK <= 5;
    rows_times_cols<T, NK, NRB, 1, kAhead ? NRB : 1, true>(lds + cur * kKimg, qf, c, g, s, cs);   // s = q.k - LSE
    const bool edge = key0 + KT > N;   // uniform: only the last tile has dead keys
#pragma unroll
    for (int kb = 0; kb < NRB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = fast_exp2(s[kb][0][r]) * Tr::to_f32(dpf[kb][r]);
        part += (!edge || key0 + kb * 16 + 4 * g + r < N) ? t : 0.f;
      }
    __syncthreads();   // K buffer `cur` is free again
  }
  const float r = quad_sum(part);
  if (g == 0 && q < N) rowdot[pair * N + q] = r;
}

// =================================================================================================== host side
// LDS tile buffers: double-buffered for the 16-bit types at head sizes <= 80 (the long-sequence layers, where the
// prefetch matters); single-buffered otherwise so that D = 160 and the f32 build fit in 160 KB
template <typename T, int NK>
struct Bufs {
  static constexpr int value = (sizeof(T) == 2 && NK <= 5) ? 2 : 1;
};
template <typename T, int NK, int KT>
size_t fwd_lds() { return sizeof(T) * Bufs<T, NK>::value * (row_img<T, NK, KT>() + col_img<T, NK, KT>()); }
template <typename T, int NK, int KT>
size_t dq_lds() { return sizeof(T) * Bufs<T, NK>::value * (2 * row_img<T, NK, KT>() + col_img<T, NK, KT>()); }
template <typename T, int NK, int KT>
size_t dkdv_lds() {
  return sizeof(T) * Bufs<T, NK>::value * (2 * row_img<T, NK, KT>() + 2 * col_img<T, NK, KT>()) + sizeof(float) * 4 * KT;
}

constexpr size_t kLdsLimit = 160 * 1024;

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
template <typename... P>
bool al16(const void* p, P... more) { return al16(p) && al16(more...); }

// What an entry point hands to its launcher once its checks have passed; what the entry does not have stays null.
struct Call {
  const void *Q, *K, *V, *O, *dO, *dP;
  const float* LSE;
  void *O_out, *P, *dQ, *dK, *dV;
  float *LSE_out, *delta, *rowdot;
  size_t dp_stride;
  int dp_vec_ok, B, H, N, D, ldq;
  float scale;
  hipStream_t s;
};
// (sizes, row stride of Q / K / V, scale and stream: the part every entry fills the same way)
Call make_call(int B, int H, int N, int D, int ld_qkv, float scale, ga_stream_t stream) {
  Call c{};
  c.B = B, c.H = H, c.N = N, c.D = D, c.ldq = ld_qkv > 0 ? ld_qkv : H * D, c.scale = scale;
  c.s = static_cast<hipStream_t>(stream);
  return c;
}

template <typename T>
struct TypeTag {
  using type = T;
};
template <int V>
struct Int {
  static constexpr int value = V;
};

// Columns (queries, or keys in dk_dv) per wave = 16 * CB.  CB = 2 halves the LDS operand traffic per MFMA but needs
// more registers and halves the number of workgroups; at batch 1 the 64x64 layer only has 2048 column blocks in
// all.  Measured (fp16, us, final round-1 kernels):
//   forward   4096x40: B=1 CB=1 65.9 / CB=2 62.8;  B=2 CB=2 97 (CB=1 ~128);  1024x80: B=3 CB=1 28.6 / CB=2 23.6
//             (384 workgroups of 86 KB LDS = two rounds of one per CU), B<=2 CB=1 better
//   backward  4096x40: B=1 CB=1 236 / CB=2 245
// Hence CB = 2 from 192 column-block pairs per launch in the forward, from 512 in the backward (round 3 read the two
// thresholds from the environment for the A/B runs: +-0.5 % either way).  launch(Int<CB>) is the launcher to run; the
// backward with and without a dP choose alike, so that a zero dP reproduces ga_self_attn_bwd bit for bit at every size.
template <int NK, typename F>
int with_columns(const Call& c, bool backward, F&& launch) {
  if constexpr (NK <= 5) {
    if ((long long)c.B * c.H * ((c.N + 127) / 128) >= (backward ? 512 : 192)) return launch(Int<2>{});
  }
  return launch(Int<1>{});
}

template <typename T, int NK, int QB>
int launch_fwd(const Call& c) {
  // 128-key tiles for the 16-query forward at small head sizes (register budget allows it), 64 otherwise
  constexpr int KT = (QB == 1 && NK <= 5 && sizeof(T) == 2) ? 128 : 64;
  constexpr int NW = 4;   // waves per workgroup (a template parameter of the kernel: tools pick kernels by the full name)
  const size_t lds = fwd_lds<T, NK, KT>();
  if (lds > kLdsLimit) return GA_ERR_SHAPE;
  const int nqt = (c.N + 16 * NW * QB - 1) / (16 * NW * QB);
  // the row sum rides on the P.V product when the head size leaves a pad column in the V image (D % 16 == 8)
  constexpr bool kCanOnes = sizeof(T) == 2 && (NK & 1);   // head sizes 8, 24, 40, 72: the odd chunk counts built here
  auto k = self_attn_fwd_kernel<T, NK, QB, Bufs<T, NK>::value, KT, false, NW>;
  if constexpr (kCanOnes) {
    if ((c.D & 15) != 0) k = self_attn_fwd_kernel<T, NK, QB, Bufs<T, NK>::value, KT, true, NW>;
  }
  int rc = set_dyn_lds(k, lds);
  if (rc != GA_OK) return rc;
  hipLaunchKernelGGL(k, dim3((unsigned)(c.B * c.H * nqt)), dim3(64 * NW), lds, c.s, (const T*)c.Q, (const T*)c.K,
                     (const T*)c.V, (T*)c.O_out, c.LSE_out, c.H, c.N, c.D, nqt, c.ldq, c.scale);
  return check_launch();
}

// The backward: dQ (fills delta), then dK + dV; with a cotangent on the probabilities (HAS_DP) the row pre-pass first and
// the dP forms of the same two bodies.
template <typename T, int NK, int CB, bool HAS_DP>
int launch_bwd(const Call& c) {
  if constexpr (HAS_DP && sizeof(T) == 4 && NK > 5) {
    return GA_ERR_UNSUPPORTED;
  } else {
    constexpr int KT = 64, NB = Bufs<T, NK>::value;
    const size_t l0 = sizeof(T) * 2 * row_img<T, NK, KT>(), l1 = dq_lds<T, NK, KT>(), l2 = dkdv_lds<T, NK, KT>();
    if ((HAS_DP && l0 > kLdsLimit) || l1 > kLdsLimit || l2 > kLdsLimit) return GA_ERR_SHAPE;
    const int nr = (c.N + 63) / 64, nt = (c.N + 64 * CB - 1) / (64 * CB), nk = (c.N + 63) / 64;
    const T *Q = (const T*)c.Q, *K = (const T*)c.K, *V = (const T*)c.V, *O = (const T*)c.O, *dO = (const T*)c.dO;
    const dim3 gq((unsigned)(c.B * c.H * nt)), gk((unsigned)(c.B * c.H * nk)), block(kThreads);
    int rc;
    if constexpr (HAS_DP) {
      auto kr = self_attn_rowdot_kernel<T, NK>;
      auto kq = self_attn_bwd_dp_dq_kernel<T, NK, CB, NB, KT>;
      auto kk = self_attn_bwd_dp_dkdv_kernel<T, NK, 1, NB, KT>;
      if ((rc = set_dyn_lds(kr, l0)) != GA_OK || (rc = set_dyn_lds(kq, l1)) != GA_OK || (rc = set_dyn_lds(kk, l2)) != GA_OK)
        return rc;
      const T* dP = (const T*)c.dP;
      hipLaunchKernelGGL(kr, dim3((unsigned)(c.B * c.H * nr)), block, l0, c.s, Q, K, dP, c.dp_stride, c.dp_vec_ok, c.LSE,
                         c.rowdot, c.H, c.N, c.D, nr, c.ldq, c.scale);
      hipLaunchKernelGGL(kq, gq, block, l1, c.s, Q, K, V, O, dO, dP, c.dp_stride, c.dp_vec_ok, c.LSE, c.delta,
                         (const float*)c.rowdot, (T*)c.dQ, c.H, c.N, c.D, nt, c.ldq, c.scale);
      hipLaunchKernelGGL(kk, gk, block, l2, c.s, Q, K, V, dO, dP, c.dp_stride, c.LSE, (const float*)c.delta,
                         (const float*)c.rowdot, (T*)c.dK, (T*)c.dV, c.H, c.N, c.D, nk, c.ldq, c.scale);
    } else {
      auto kq = self_attn_bwd_dq_kernel<T, NK, CB, NB, KT>;
      auto kk = self_attn_bwd_dkdv_kernel<T, NK, 1, NB, KT>;  // dk_dv: 16 keys per wave (register budget)
      if ((rc = set_dyn_lds(kq, l1)) != GA_OK || (rc = set_dyn_lds(kk, l2)) != GA_OK) return rc;
      hipLaunchKernelGGL(kq, gq, block, l1, c.s, Q, K, V, O, dO, c.LSE, c.delta, (T*)c.dQ, c.H, c.N, c.D, nt, c.ldq, c.scale);
      hipLaunchKernelGGL(kk, gk, block, l2, c.s, Q, K, V, dO, c.LSE, (const float*)c.delta, (T*)c.dK, (T*)c.dV, c.H, c.N,
                         c.D, nk, c.ldq, c.scale);
    }
    return check_launch();
  }
}

template <typename T, int NK>
int launch_probs(const Call& c) {
  if constexpr (sizeof(T) == 4 && NK > 5) {
    return GA_ERR_UNSUPPORTED;
  } else {
    constexpr int KT = 64;
    const size_t lds = sizeof(T) * (2 * row_img<T, NK, KT>() + 4 * 16 * (KT + TL<T, KT>::VEC));
    if (lds > kLdsLimit) return GA_ERR_SHAPE;
    const int nqt = (c.N + 63) / 64;
    const int vec_ok = al16(c.P) && ((size_t)c.N * sizeof(T)) % 16 == 0;
    auto k = self_attn_probs_kernel<T, NK>;
    int rc = set_dyn_lds(k, lds);
    if (rc != GA_OK) return rc;
    hipLaunchKernelGGL(k, dim3((unsigned)(c.B * c.H * nqt)), dim3(kThreads), lds, c.s, (const T*)c.Q, (const T*)c.K, c.LSE,
                       (T*)c.P, c.H, c.N, c.D, nqt, c.ldq, c.scale, vec_ok);
    return check_launch();
  }
}

// The one dispatch over element type and head-size class: run(TypeTag<T>, Int<NK>), NK = 16-wide chunks of the padded head size.
template <typename T, typename F>
int by_head_size(int D, F&& run) {
  const int nk = (D + 15) / 16;
  if (nk <= 1) return run(TypeTag<T>{}, Int<1>{});
  if (nk == 2) return run(TypeTag<T>{}, Int<2>{});
  if (nk == 3) return run(TypeTag<T>{}, Int<3>{});
  if (nk == 4) return run(TypeTag<T>{}, Int<4>{});
  if (nk == 5) return run(TypeTag<T>{}, Int<5>{});
  if (nk <= 8) return run(TypeTag<T>{}, Int<8>{});
  if (nk <= 10) return run(TypeTag<T>{}, Int<10>{});
  return GA_ERR_SHAPE;
}
template <typename F>
int dispatch(int dtype, int D, F&& run) {
#ifdef GA_SA_MICRO   /* micro-benchmark builds (tools/sa_variants.py): f16 and one head-size class, fast to compile */
  if (dtype != GA_F16) return GA_ERR_DTYPE;
  return (D + 15) / 16 == GA_SA_MICRO ? run(TypeTag<_Float16>{}, Int<GA_SA_MICRO>{}) : GA_ERR_SHAPE;
#else
  switch (dtype) {
    case GA_F16: return by_head_size<_Float16>(D, run);
    case GA_BF16: return by_head_size<bf16_t>(D, run);
    case GA_F32: return by_head_size<float>(D, run);
    default: return GA_ERR_DTYPE;
  }
#endif
}
// inside a run(t, nk) / launch(cb) lambda: the type and the integers the tags stand for
#define GA_T typename decltype(t)::type
#define GA_V(x) decltype(x)::value

int check_args(int B, int H, int N, int D) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0 || D > 160) return GA_ERR_SHAPE;
  if (D % 8 != 0) return GA_ERR_ALIGN;
  if ((long long)B * H * ((N + 63) / 64) > 0x7fffffffLL) return GA_ERR_SHAPE;
  return GA_OK;
}
// ga_self_attn_fwd / _bwd: the dtype is looked at last (by the dispatch); any row stride that holds a row and keeps it aligned.
int check_args_any_stride(int B, int H, int N, int D, int ld_qkv) {
  int rc = check_args(B, H, N, D);
  if (rc != GA_OK) return rc;
  const int ldq = ld_qkv > 0 ? ld_qkv : H * D;
  return (ldq < H * D || ldq % 8 != 0) ? GA_ERR_SHAPE : GA_OK;
}
// The probability entries and the dP backward: the dtype first; ld_qkv is 0 (dense) or 3 H D (slices of one fused QKV tensor).
int check_args_fused_stride(int B, int H, int N, int D, int ld_qkv, int dtype) {
  if (dtype != GA_F16 && dtype != GA_BF16 && dtype != GA_F32) return GA_ERR_DTYPE;
  int rc = check_args(B, H, N, D);
  if (rc != GA_OK) return rc;
  if (dtype == GA_F32 && D > 80) return GA_ERR_UNSUPPORTED;
  if (ld_qkv != 0 && (long long)ld_qkv != 3LL * H * D) return GA_ERR_SHAPE;
  return GA_OK;
}
bool elem_aligned(const void* p, int dtype) { return reinterpret_cast<uintptr_t>(p) % (dtype == GA_F32 ? 4 : 2) == 0; }

// What both probability entries check before any launch.
int check_probs_args(const void* Q, const void* K, const float* LSE, const void* P, int B, int H, int N, int D,
                     int ld_qkv, int dtype) {
  if (!Q || !K || !LSE || !P) return GA_ERR_NULL;
  int rc = check_args_fused_stride(B, H, N, D, ld_qkv, dtype);
  if (rc != GA_OK) return rc;
  return al16(Q, K) && elem_aligned(P, dtype) ? GA_OK : GA_ERR_ALIGN;
}

}  // namespace

extern "C" int ga_self_attn_fwd(const void* Q, const void* K, const void* V, void* O, float* LSE, int B, int H, int N,
                                int D, int ld_qkv, float scale, int dtype, ga_stream_t stream) {
  if (!Q || !K || !V || !O) return GA_ERR_NULL;
  int rc = check_args_any_stride(B, H, N, D, ld_qkv);
  if (rc != GA_OK) return rc;
  if (!al16(Q, K, V, O)) return GA_ERR_ALIGN;
  Call c = make_call(B, H, N, D, ld_qkv, scale, stream);
  c.Q = Q, c.K = K, c.V = V, c.O_out = O, c.LSE_out = LSE;
  return dispatch(dtype, D, [&](auto t, auto nk) {
    return with_columns<GA_V(nk)>(c, false, [&](auto qb) { return launch_fwd<GA_T, GA_V(nk), GA_V(qb)>(c); });
  });
}

extern "C" int ga_self_attn_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO,
                                const float* LSE, float* delta, void* dQ, void* dK, void* dV, int B, int H, int N,
                                int D, int ld_qkv, float scale, int dtype, ga_stream_t stream) {
  if (!Q || !K || !V || !O || !dO || !LSE || !delta || !dQ || !dK || !dV) return GA_ERR_NULL;
  int rc = check_args_any_stride(B, H, N, D, ld_qkv);
  if (rc != GA_OK) return rc;
  if (!al16(Q, K, V, O, dO, dQ, dK, dV)) return GA_ERR_ALIGN;
  Call c = make_call(B, H, N, D, ld_qkv, scale, stream);
  c.Q = Q, c.K = K, c.V = V, c.O = O, c.dO = dO, c.LSE = LSE, c.delta = delta, c.dQ = dQ, c.dK = dK, c.dV = dV;
  return dispatch(dtype, D, [&](auto t, auto nk) {
    return with_columns<GA_V(nk)>(c, true, [&](auto cb) { return launch_bwd<GA_T, GA_V(nk), GA_V(cb), false>(c); });
  });
}

extern "C" int ga_self_attn_bwd_dp(const void* Q, const void* K, const void* V, const void* O, const void* dO,
                                   const void* dP, int64_t dp_map_stride, const float* LSE, float* delta, float* rowdot,
                                   void* dQ, void* dK, void* dV, int B, int H, int N, int D, int ld_qkv, float scale,
                                   int dtype, ga_stream_t stream) {
  // everything before the first launch; O and dO come together or not at all (the loss read the probabilities only)
  if (!Q || !K || !V || !dP || !LSE || !delta || !rowdot || !dQ || !dK || !dV || (O == nullptr) != (dO == nullptr))
    return GA_ERR_NULL;
  int rc = check_args_fused_stride(B, H, N, D, ld_qkv, dtype);
  if (rc != GA_OK) return rc;
  if (dp_map_stride < 0 || (dp_map_stride != 0 && dp_map_stride < (int64_t)N * N)) return GA_ERR_SHAPE;
  if (!al16(Q, K, V, dQ, dK, dV) || (O && !al16(O, dO)) || !elem_aligned(dP, dtype)) return GA_ERR_ALIGN;
  Call c = make_call(B, H, N, D, ld_qkv, scale, stream);
  c.Q = Q, c.K = K, c.V = V, c.O = O, c.dO = dO, c.dP = dP, c.LSE = LSE, c.delta = delta, c.rowdot = rowdot;
  c.dQ = dQ, c.dK = dK, c.dV = dV, c.dp_stride = (size_t)dp_map_stride;
  // a lane's run of four consecutive keys is one load when every run of every map starts on a four-element boundary
  c.dp_vec_ok = reinterpret_cast<uintptr_t>(dP) % (dtype == GA_F32 ? 16 : 8) == 0 && N % 4 == 0 && dp_map_stride % 4 == 0;
  return dispatch(dtype, D, [&](auto t, auto nk) {
    return with_columns<GA_V(nk)>(c, true, [&](auto cb) { return launch_bwd<GA_T, GA_V(nk), GA_V(cb), true>(c); });
  });
}

extern "C" int ga_self_attn_probs(const void* Q, const void* K, const float* LSE, void* P, int B, int H, int N, int D,
                                  int ld_qkv, float scale, int dtype, ga_stream_t stream) {
  int rc = check_probs_args(Q, K, LSE, P, B, H, N, D, ld_qkv, dtype);
  if (rc != GA_OK) return rc;
  Call c = make_call(B, H, N, D, ld_qkv, scale, stream);
  c.Q = Q, c.K = K, c.LSE = LSE, c.P = P;
  return dispatch(dtype, D, [&](auto t, auto nk) { return launch_probs<GA_T, GA_V(nk)>(c); });
}

extern "C" int ga_self_attn_capture_fwd(const void* Q, const void* K, const void* V, void* O, float* LSE, void* P, int B,
                                        int H, int N, int D, int ld_qkv, float scale, int dtype, ga_stream_t stream) {
  if (!V || !O) return GA_ERR_NULL;
  int rc = check_probs_args(Q, K, LSE, P, B, H, N, D, ld_qkv, dtype);   // everything, before the first launch
  if (rc != GA_OK) return rc;
  if (!al16(V, O)) return GA_ERR_ALIGN;
  rc = ga_self_attn_fwd(Q, K, V, O, LSE, B, H, N, D, ld_qkv, scale, dtype, stream);
  if (rc != GA_OK) return rc;
  return ga_self_attn_probs(Q, K, LSE, P, B, H, N, D, ld_qkv, scale, dtype, stream);
}

#undef GA_T
#undef GA_V
