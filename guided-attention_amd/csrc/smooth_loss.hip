// K3+K4: the Gaussian-smoothed bounding-box loss over the aggregated maps A (res, res, Kt), forward
// and analytic backward.  Replaces the reference's per-pixel Python loops
// (pipeline_guided_attention.py:201-296,359-451; utils/helpers.py:164-173,215-277;
// utils/gaussian_smoothing.py:21-71).
//
// The whole problem is 16*16*77 floats (79 KB): it is launch-latency bound, not bandwidth bound, so
// it runs as ONE 256-thread workgroup that keeps every intermediate in LDS, walks the guided tokens
// sequentially (deterministic reductions, no atomics) and touches HBM once per input element.
//
//   S[p][j]  = softmax_j(100 * A[p][first + j]),  j in [0, last-first)
//   per guided token k:  M = S[:, k] -> M' = reflect-pad Gaussian smoothing -> s = sum M', Pn = M'/s
//       col = sum (j+.5) Pn, row = sum (i+.5) Pn, inside = 1 - sum_in Pn, outside = sum_out Pn
//       item = w_in*inside + 3*w_out*outside + w_c*(|col - res*cx| + 4|row - res*cy|)/(res-1)
//   loss = sum_k weight_k * item_k
// strict mode (curHyperParams["strict"], helpers.py:216-264): a per-pixel weight table W (inside: np.interp of the
// normalised distance from the box centre, outside: 1; normalised separately over the inside and the outside pixels)
// and hinge terms  inside = sum_in W * 2*max(0, 1/n_in - Pn),  outside = sum_out W * max(0, Pn).
// The reference hard-codes res = 16 ("16", "15."); res and res-1 are used here (identical at 16).
#include "aggregate.h"
#include "attn_common.h"

using namespace ga;

namespace {

constexpr int kMaxTok = 32;
constexpr int kMaxK = 7;
constexpr int kThreads = 256;

static_assert(kMaxTok == GA_IMAGE_MAX_TOKENS, "one descriptor row holds every token a launch can guide");
static_assert(sizeof(ga_image_loss_t) == 1576, "ga_image_loss_t layout");

// The relation losses (toLeftOf, toRightOf, above, below) of the *_rel_* launches.  An image's relation tokens — (relation, side, position): 4 x 2 x 8, one
// lane of wave 0 each — name at most Q_max DISTINCT slice indices; each gets a slot behind the T_max guided-token slots of
// gcol and dS.  Everything the relation work shares between threads lives in this block of LDS behind the two staged rows.
constexpr int kMaxRelCols = 32;
constexpr int kRelToks = GA_IMAGE_MAX_RELATIONS * 2 * GA_REL_MAX_TOKENS;
static_assert(kRelToks == 64, "one lane of a wave per relation token");
static_assert(sizeof(ga_relation_t) == 80 && sizeof(ga_image_relations_t) == 336, "relation row layout");
static_assert(kMaxRelCols <= 128 && kMaxTok <= 128, "slots fit a signed byte");
struct RelLds {
  int ok, nq, any_open, _pad;
  int qcol[kMaxRelCols];            // slice index of slot q
  signed char merged[kMaxRelCols];  // the guided-token slot that has slot q's column, or -1
  signed char tokslot[kRelToks];    // slot of relation token (r * 2 + side) * 8 + k, -1: unused
  int _free[8];                     // keeps the block at the 960 bytes the hosts' LDS plans were pinned with
  float m[kMaxRelCols];                     // mass of slot q
  float c[kMaxRelCols], cy[kMaxRelCols];    // its centroid column and centroid row
  float w[kMaxRelCols], wy[kMaxRelCols];    // d loss / d centroid column, d loss / d centroid row
  float v[GA_IMAGE_MAX_RELATIONS], cL[GA_IMAGE_MAX_RELATIONS], cR[GA_IMAGE_MAX_RELATIONS];   // cL: the "left" role's sum
};
static_assert(sizeof(RelLds) == 960, "the relation front is ROW_BYTES + 336 + 960: a larger block moves the LDS plans");
// the axis and the role of a relation kind (ga_hip.h): the centroid row instead of the centroid column; right[] instead of
// left[] plays the reference's "left" role (added, and its count divides both sums)
__device__ __forceinline__ bool rel_vertical(int kind) { return kind == GA_REL_ABOVE || kind == GA_REL_BELOW; }
__device__ __forceinline__ int rel_lead_side(int kind) { return (kind == GA_REL_RIGHT_OF || kind == GA_REL_BELOW) ? 1 : 0; }
constexpr int kRelRowFloats = (int)((sizeof(ga_image_relations_t) + 15) / 16 * 4);
constexpr int kRelLdsFloats = (int)((sizeof(RelLds) + 15) / 16 * 4);
// what a *_rel_* launch hands to the loss functions next to the descriptor row; the other launches pass an empty one and
// compile none of its uses (kRel = false)
struct RelCtx {
  const ga_image_relations_t* row = nullptr;   // image blockIdx.y's relation row, staged in LDS
  RelLds* st = nullptr;
  int Q_max = 0;
  float* sm2 = nullptr;     // [npix] in LDS: the compensated sum of exponentials per pixel (row_stats<true>)
  float* terms = nullptr;   // [GA_IMAGE_MAX_RELATIONS][4] of this image
  float* loss = nullptr;    // [1] of this image
};

// Call-level arguments, plus the ONE image descriptor of the launches that take it as arguments (`img`).  The table launches
// (ga_*_images) read image blockIdx.y's descriptor from `table` in device memory instead; every loss function below takes
// the descriptor `d` it works on as a separate reference, so both forms run the same code.
struct LossArgs {
  const float* A;
  long long img_stride;   // elements between two images' maps: the image of a workgroup is blockIdx.y (batched launches)
  int res, Kt;
  int T_max;        // LDS tables and terms rows are sized for this many tokens (== img.T for the argument form)
  int ksize, smooth;
  int w_lds;        // the strict-mode weight table W has LDS (some image may be strict)
  int stage_rows;   // pixel rows of A staged through LDS per pass of the softmax statistics (0: read from global memory)
  int use_gcol;     // the guided tokens' columns of A are kept in LDS ([T_max][npix]); 0 (LDS budget): re-read from global memory
  float gw[kMaxK * kMaxK];
  const ga_image_loss_t* table;   // [images] rows in device memory, or NULL: every image uses `img`
  ga_image_loss_t img;
};

// the loss weights of a descriptor as the loss math uses them (the argument form used to precompute these on the host:
// the same single fp32 operations)
__device__ __forceinline__ float w_out3(const ga_image_loss_t& d) { return d.outside_scale * 3.0f; }

__device__ __forceinline__ int reflect_idx(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// helpers.py:164-173 inside_box at pixel centre (j+.5, i+.5); float64, same operation order as the
// reference (each product / sum rounded separately: no FMA contraction)
__device__ __forceinline__ bool inside_box(const ga_token_t& t, int res, double shrink, int i, int j) {
  const double ratio = (double)res;  // Rect.of_size: float(new_size / size), size = 1
  const double x = __dmul_rn(t.geom[0], ratio), y = __dmul_rn(t.geom[1], ratio);
  const double w = __dmul_rn(t.geom[2], ratio), h = __dmul_rn(t.geom[3], ratio);
  const double ox = __dmul_rn(shrink, w), oy = __dmul_rn(shrink, h);
  const double cx = (double)j + 0.5, cy = (double)i + 0.5;
  if (cx >= __dadd_rn(x, ox) && cx <= __dsub_rn(__dadd_rn(x, w), ox))
    if (cy >= __dadd_rn(y, oy) && cy <= __dsub_rn(__dadd_rn(y, h), oy)) return true;
  return false;
}

// block-wide sum of NV values per thread; result valid in every thread.  scratch: [4][NV] floats.
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* scratch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_reduce_sum(v[k]);
  __syncthreads();  // scratch may still be read from a previous call
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) scratch[wave * NV + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = (scratch[k] + scratch[NV + k]) + (scratch[2 * NV + k] + scratch[3 * NV + k]);
}

__device__ __forceinline__ float block_max(float v, float* scratch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_reduce_max(v);
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  return fmaxf(fmaxf(scratch[0], scratch[1]), fmaxf(scratch[2], scratch[3]));
}

// per-pixel softmax statistics of 100*A over the text slice: row max and sum of exponentials, each row summed in token
// order by ONE thread (the order the fixtures of the reference's fp32 softmax were matched with: a tree-ordered sum moves
// the near-one-hot rows by more than the 3e-5 bar after the x100 backward).  The rows are staged through LDS in chunks
// of `stage_rows` pixels with coalesced 16-byte loads (a chunk of A is contiguous), and a thread then walks its row in LDS
// (row stride Kt words: conflict-free for the odd Kt of the text context).  Walking the rows straight from global memory
// — 64 different cache lines per load instruction, 150 dependent-latency loads per thread — was most of the 35 us the
// single-workgroup kernel took in round 2; `stage_rows` = 0 (maps too large for the LDS budget) keeps that form.
__device__ __forceinline__ float* align16(float* p) {
  return reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(p) + 15) & ~(uintptr_t)15);
}

// kAcc (the *_rel_* launches): `s2_out` is the same sum with its rounding errors carried along (TwoSum per addition).  The
// token-order sum of a near-one-hot row drops most of what the small exponentials add to the 1 of the row's maximum — up to
// (last - first) * 2^-25 — and 1 - S of that row is what the relation's gradient is made of at such a pixel.  The box terms
// keep the token-order sum (s_out: the reference's numbers were matched with it).
template <bool kAcc = false>
__device__ __forceinline__ void row_stats(const ga_image_loss_t& a, const float* row, float& m_out, float& s_out,
                                          float* s2_out = nullptr) {
  // eight reads in flight per trip; the maximum and the sum still run in token order (one thread, one row).  The plain
  // `for c: m = max(m, row[c] * 100)` loop paid a full LDS round trip per element: 15 us of the launch for 256 rows.
  float m = -INFINITY;
  for (int c0 = a.first; c0 < a.last; c0 += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = row[min(c0 + u, a.last - 1)] * 100.0f;
#pragma unroll
    for (int u = 0; u < 8; ++u) m = fmaxf(m, v[u]);          // the clamped repeats of the last element change nothing
  }
  float s = 0.f, lo = 0.f;
  for (int c0 = a.first; c0 < a.last; c0 += 8) {
    float e[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) e[u] = expf(row[min(c0 + u, a.last - 1)] * 100.0f - m);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (c0 + u < a.last) {
        if constexpr (kAcc) {
          const float t = s + e[u], bp = t - s;
          lo += (s - (t - bp)) + (e[u] - bp);
        }
        s += e[u];
      }
  }
  m_out = m;
  s_out = s;
  if constexpr (kAcc) *s2_out = s + lo;
}

// gcol[t][p] = A[p][column of guided token t]: taken while the row is at hand, so that the token loops never go back to
// global memory (one dependent ~1-2 us load per token and phase otherwise: the launch is one workgroup, nothing hides it)
template <bool kRel>
__device__ __forceinline__ void gather_guided(const LossArgs& a, const ga_image_loss_t& d, const RelCtx& rc, const float* row,
                                              int p, int npix, float* gcol) {
  if (!a.use_gcol) return;
  for (int t = 0; t < d.T; ++t) gcol[t * npix + p] = row[d.first + d.tok[t].token - 1];
  if constexpr (kRel)
    for (int q = 0; q < rc.st->nq; ++q) gcol[(a.T_max + q) * npix + p] = row[d.first + rc.st->qcol[q]];
}
// this workgroup's image of A: grid.y is 1 for the single-image entry points, S for the batched ones
__device__ __forceinline__ const float* image_A(const LossArgs& a) { return a.A + (size_t)blockIdx.y * a.img_stride; }
// A[p][column of guided token t]
__device__ __forceinline__ float guided_value(const LossArgs& a, const ga_image_loss_t& d, const float* gcol, int t, int p,
                                              int npix) {
  return a.use_gcol ? gcol[(size_t)t * npix + p] : image_A(a)[(size_t)p * a.Kt + d.first + d.tok[t].token - 1];
}
// A[p][column of relation slot q]
__device__ __forceinline__ float rel_value(const LossArgs& a, const ga_image_loss_t& d, const RelCtx& rc, const float* gcol,
                                           int q, int p, int npix) {
  return a.use_gcol ? gcol[(size_t)(a.T_max + q) * npix + p] : image_A(a)[(size_t)p * a.Kt + d.first + rc.st->qcol[q]];
}

template <bool kRel>
__device__ __forceinline__ void pixel_softmax_stats(const LossArgs& a, const ga_image_loss_t& d, const RelCtx& rc, float* mx,
                                                    float* sm, float* stage, float* gcol) {
  const int npix = a.res * a.res;
  if (a.stage_rows == 0) {
    for (int p = threadIdx.x; p < npix; p += kThreads) {
      if constexpr (kRel)
        row_stats<true>(d, image_A(a) + (size_t)p * a.Kt, mx[p], sm[p], rc.sm2 + p);
      else
        row_stats(d, image_A(a) + (size_t)p * a.Kt, mx[p], sm[p]);
      gather_guided<kRel>(a, d, rc, image_A(a) + (size_t)p * a.Kt, p, npix, gcol);
    }
    return;
  }
  for (int p0 = 0; p0 < npix; p0 += a.stage_rows) {
    const int rows = min(a.stage_rows, npix - p0), n = rows * a.Kt;
    const float* src = image_A(a) + (size_t)p0 * a.Kt;   // 16-byte aligned: stage_rows is a multiple of 4, A is (and so
    // is every image of a batched A: the host stages nothing when npix * Kt is not a multiple of 4)
    // eight 16-byte loads per thread in flight before the first LDS store (a load -> store loop pays one memory round
    // trip per iteration: 19 of them for the 16 x 16 x 77 map, most of what this launch took)
    for (int e0 = 0; e0 + 3 < n; e0 += 4 * kThreads * 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 4 * (threadIdx.x + u * kThreads);
        v[u] = *reinterpret_cast<const f32x4*>(src + min(e, (n & ~3) - 4));
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 4 * (threadIdx.x + u * kThreads);
        if (e + 3 < n) *reinterpret_cast<f32x4*>(stage + e) = v[u];
      }
    }
    for (int e = (n & ~3) + threadIdx.x; e < n; e += kThreads) stage[e] = src[e];
    __syncthreads();
    for (int r = threadIdx.x; r < rows; r += kThreads) {
      if constexpr (kRel)
        row_stats<true>(d, stage + r * a.Kt, mx[p0 + r], sm[p0 + r], rc.sm2 + p0 + r);
      else
        row_stats(d, stage + r * a.Kt, mx[p0 + r], sm[p0 + r]);
      gather_guided<kRel>(a, d, rc, stage + r * a.Kt, p0 + r, npix, gcol);
    }
    __syncthreads();
  }
}

struct TokenStats {
  float s, mxv, col, row, in, out, at_most;
};

// helpers.py:159-162 get_corresponding_weight = np.interp(x, [0, .333, .666, 1], [3, 2.5, 1, .2]) in float64
__device__ __forceinline__ double interp_weight(double x) {
  const double xp[4] = {0.0, .333, .666, 1.0}, fp[4] = {3.0, 2.5, 1.0, .2};
  if (x <= xp[0]) return fp[0];
  if (x >= xp[3]) return fp[3];
  int j = 0;
  while (j < 2 && x >= xp[j + 1]) ++j;
  const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
  return slope * (x - xp[j]) + fp[j];
}

// helpers.py:216-246: the strict-mode weight table of one BOX token into W[npix] (LDS), normalised separately over
// the inside and the outside pixels; the two sums run in pixel order in fp32 like the reference's (one thread: 256 to
// 4096 adds, strict mode is off by default).  Returns 1/n_inside rounded to fp32 (`at_most`, helpers.py:249).
__device__ __forceinline__ float strict_weights(const LossArgs& a, const ga_image_loss_t& d, const ga_token_t& tk, float* W,
                                                float* scratch) {
  const int res = a.res, npix = res * res;
  const double ratio = (double)res;
  const double x = __dmul_rn(tk.geom[0], ratio), y = __dmul_rn(tk.geom[1], ratio);
  const double w = __dmul_rn(tk.geom[2], ratio), h = __dmul_rn(tk.geom[3], ratio);
  const double ccx = __dadd_rn(x, w / 2.0), ccy = __dadd_rn(y, h / 2.0);  // Rect.center() of the scaled rect
  for (int p = threadIdx.x; p < npix; p += kThreads) {
    const int i = p / res, j = p - i * res;
    float wv = 1.0f;  // outside: get_corresponding_weight_distance_from == 1
    if (inside_box(tk, res, d.shrink, i, j)) {
      const double dx = __ddiv_rn(__dmul_rn(2.0, __dsub_rn(ccx, (double)j + 0.5)), w);
      const double dy = __ddiv_rn(__dmul_rn(2.0, __dsub_rn(ccy, (double)i + 0.5)), h);
      const double d = __ddiv_rn(__dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy))), __dsqrt_rn(2.0));
      wv = (float)interp_weight(d);
    }
    W[p] = wv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s_in = 0.f, s_out = 0.f;
    int n_in = 0;
    for (int p = 0; p < npix; ++p) {
      const int i = p / res, j = p - i * res;
      if (inside_box(tk, res, d.shrink, i, j)) {
        s_in += W[p];
        ++n_in;
      } else {
        s_out += W[p];
      }
    }
    scratch[0] = s_in;
    scratch[1] = s_out;
    scratch[2] = (float)(1.0 / (double)n_in);
  }
  __syncthreads();
  const float s_in = scratch[0], s_out = scratch[1], at_most = scratch[2];
  for (int p = threadIdx.x; p < npix; p += kThreads) {
    const int i = p / res, j = p - i * res;
    W[p] = W[p] / (inside_box(tk, res, d.shrink, i, j) ? s_in : s_out);
  }
  __syncthreads();
  return at_most;
}

// Forward of one token into LDS: M (raw map), Pn (smoothed, normalised).  Returns the reductions.
__device__ __forceinline__ TokenStats token_forward(const LossArgs& a, const ga_image_loss_t& d, const ga_token_t& tk,
                                                    const float* mx, const float* sm, const float* gcol, int t_idx, float* M,
                                                    float* Pn, float* W, float* scratch) {
  const int res = a.res, npix = res * res;
  const bool strict = d.strict && tk.kind == GA_TOK_BOX;
  float at_most = 0.f;
  if (strict) at_most = strict_weights(a, d, tk, W, scratch);
  // A[p][first + token - 1]  (pipeline:228 "index - 1" into the [first:last) slice)
  for (int p = threadIdx.x; p < npix; p += kThreads) M[p] = expf(guided_value(a, d, gcol, t_idx, p, npix) * 100.0f - mx[p]) / sm[p];
  __syncthreads();
  const int pad = a.ksize >> 1;
  float v2[2] = {0.f, 0.f};
  float vmax = -INFINITY;
  for (int p = threadIdx.x; p < npix; p += kThreads) {
    float acc;
    if (a.smooth) {
      const int i = p / res, j = p - i * res;
      acc = 0.f;
      for (int u = 0; u < a.ksize; ++u) {
        const int ii = reflect_idx(i + u - pad, res);
        for (int v = 0; v < a.ksize; ++v) acc += a.gw[u * a.ksize + v] * M[ii * res + reflect_idx(j + v - pad, res)];
      }
    } else {
      acc = M[p];
    }
    Pn[p] = acc;
    v2[0] += acc;
    vmax = fmaxf(vmax, acc);
  }
  block_sum<2>(v2, scratch);
  TokenStats st;
  st.s = v2[0];
  st.mxv = block_max(vmax, scratch);
  float v4[4] = {0.f, 0.f, 0.f, 0.f};
  for (int p = threadIdx.x; p < npix; p += kThreads) {
    const int i = p / res, j = p - i * res;
    const float pn = Pn[p] / st.s;
    Pn[p] = pn;
    v4[0] += ((float)j + 0.5f) * pn;
    v4[1] += ((float)i + 0.5f) * pn;
    if (tk.kind == GA_TOK_BOX) {
      const bool in = inside_box(tk, res, d.shrink, i, j);
      if (strict) {  // helpers.py:250-264
        if (in)
          v4[2] += W[p] * (2.0f * fmaxf(0.f, at_most - pn));
        else
          v4[3] += W[p] * fmaxf(0.f, pn);
      } else if (in) {
        v4[2] += pn;
      } else {
        v4[3] += pn;
      }
    }
  }
  block_sum<4>(v4, scratch);
  st.col = v4[0];
  st.row = v4[1];
  st.in = v4[2];
  st.out = v4[3];
  st.at_most = at_most;
  return st;
}

struct TokenLoss {
  float inside, outside, item, unscaled, dc, dr, w_in, w_out3, w_c;
};

__device__ __forceinline__ TokenLoss token_loss(const LossArgs& a, const ga_image_loss_t& d, const ga_token_t& tk,
                                                const TokenStats& st) {
  TokenLoss r;
  const float res = (float)a.res;
  float cx, cy;
  if (tk.kind == GA_TOK_BOX) {  // helpers.py:26-27 Rect.center in float64, then used against fp32 tensors
    cx = (float)(tk.geom[0] + tk.geom[2] / 2.0);
    cy = (float)(tk.geom[1] + tk.geom[3] / 2.0);
    r.inside = d.strict ? st.in : 1.0f - st.in;  // helpers.py:261 (strict) / :275
    r.outside = st.out;                          // helpers.py:263 (strict) / :276
    r.w_in = d.inside_scale;
    r.w_out3 = w_out3(d);
    r.w_c = d.center_weight > 0.f ? d.center_weight : 0.f;
  } else {
    cx = (float)tk.geom[0];
    cy = (float)tk.geom[1];
    r.inside = r.outside = 0.f;
    r.w_in = r.w_out3 = 0.f;
    r.w_c = 1.0f;
  }
  r.dc = st.col - cx * res;
  r.dr = st.row - cy * res;
  const float centering = fabsf(r.dc) / (res - 1.0f) + 4.0f * fabsf(r.dr) / (res - 1.0f);  // pipeline:391-395
  if (tk.kind == GA_TOK_BOX) {
    r.item = r.w_in * r.inside + r.w_out3 * r.outside + r.w_c * centering;  // pipeline:423-434
    r.unscaled = r.inside + r.outside;
  } else {
    r.item = r.unscaled = centering;  // pipeline:409-414
  }
  return r;
}

// The table launches copy image blockIdx.y's descriptor row into LDS before anything reads it: two loads per thread in one
// batch.  The row sits at the start of the dynamic LDS, the loss tables behind it (kRowFloats; no static LDS: set_dyn_lds
// grants the kernels the whole 160 KB as dynamic LDS).  Read in place, every token field the loss loops touch was one more load waited for alone (12 serial round trips
// in a row in the last arriver of the fused launch).
constexpr int kRowFloats = (int)((sizeof(ga_image_loss_t) + 15) / 16 * 4);
__device__ __forceinline__ const ga_image_loss_t& stage_row(const ga_image_loss_t* table, ga_image_loss_t* s) {
  constexpr int kWords = (int)(sizeof(ga_image_loss_t) / 4);
  static_assert(kWords <= 2 * kThreads, "one row: two words per thread");
  const unsigned* src = reinterpret_cast<const unsigned*>(table + blockIdx.y);
  unsigned* dst = reinterpret_cast<unsigned*>(s);
  unsigned v[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) v[u] = src[min((int)threadIdx.x + u * kThreads, kWords - 1)];
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if ((int)threadIdx.x + u * kThreads < kWords) dst[threadIdx.x + u * kThreads] = v[u];
  __syncthreads();
  return *s;
}

// A descriptor row of the table launches that the kernels cannot serve (they never read past tok[T_max - 1] nor outside the
// image's map): the image gets loss NaN and zero terms / dA.  The argument form is checked on the host (fill_args).
__device__ __forceinline__ bool row_ok(const LossArgs& a, const ga_image_loss_t& d) {
  if (d.T < 0 || d.T > a.T_max) return false;
  if (d.T == 0) return true;
  if (d.first < 0 || d.last > a.Kt || d.last - d.first < 1 || (d.strict && !a.w_lds)) return false;
  for (int t = 0; t < d.T; ++t) {
    const int col = d.first + d.tok[t].token - 1;
    if (col < d.first || col >= d.last || (d.tok[t].kind != GA_TOK_BOX && d.tok[t].kind != GA_TOK_COOR)) return false;
  }
  return true;
}

// The *_rel_* launches stage image blockIdx.y's relation row next to its loss row: three loads per thread in ONE batch.
__device__ __forceinline__ void stage_rows_rel(const ga_image_loss_t* table, const ga_image_relations_t* rel_table,
                                               ga_image_loss_t* s, ga_image_relations_t* sr) {
  constexpr int kWords = (int)(sizeof(ga_image_loss_t) / 4), kRelWords = (int)(sizeof(ga_image_relations_t) / 4);
  static_assert(kWords <= 2 * kThreads && kRelWords <= kThreads, "two words of the loss row, one of the relation row per thread");
  const unsigned* src = reinterpret_cast<const unsigned*>(table + blockIdx.y);
  const unsigned* rsrc = reinterpret_cast<const unsigned*>(rel_table + blockIdx.y);
  unsigned* dst = reinterpret_cast<unsigned*>(s);
  unsigned* rdst = reinterpret_cast<unsigned*>(sr);
  unsigned v[3];
#pragma unroll
  for (int u = 0; u < 2; ++u) v[u] = src[min((int)threadIdx.x + u * kThreads, kWords - 1)];
  v[2] = rsrc[min((int)threadIdx.x, kRelWords - 1)];
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if ((int)threadIdx.x + u * kThreads < kWords) dst[threadIdx.x + u * kThreads] = v[u];
  if ((int)threadIdx.x < kRelWords) rdst[threadIdx.x] = v[2];
  __syncthreads();
}

// Screens image blockIdx.y's relation row and numbers its distinct columns (RelLds: nq, qcol, tokslot).  One lane of wave 0
// per relation token: a token's slot is that of the lowest lane naming the same slice index.  -> the row pair can be served
// (`base_ok`: row_ok of the loss row).  Every thread of the workgroup calls it.
__device__ __forceinline__ bool rel_setup(const LossArgs& a, const ga_image_loss_t& d, const RelCtx& rc, bool base_ok) {
  const ga_image_relations_t& rq = *rc.row;
  RelLds* rl = rc.st;
  if (threadIdx.x < kRelToks) {
    const int j = threadIdx.x;
    const int r = j >> 4, side = (j >> 3) & 1, k = j & 7;
    const bool R_ok = rq.R >= 0 && rq.R <= GA_IMAGE_MAX_RELATIONS;
    const int R = R_ok ? rq.R : 0;
    const ga_relation_t& rel = rq.rel[r];
    const int n = side ? rel.n_right : rel.n_left;
    const bool used = r < R && k < n && n <= GA_REL_MAX_TOKENS;
    const int idx = used ? (side ? rel.right[k] : rel.left[k]) : -1 - j;   // unused lanes: all different, none a slice index
    const int width = d.last - d.first;
    bool bad = !R_ok;
    if (r < R && k == 0) bad |= n < 1 || n > GA_REL_MAX_TOKENS || rel.kind < GA_REL_LEFT_OF || rel.kind > GA_REL_BELOW;
    if (used) bad |= idx < 0 || idx >= width;
    if (R > 0) bad |= d.first < 0 || d.last > a.Kt || width < 1;
    int lead = j;   // the lowest lane with this slice index
    for (int jj = kRelToks - 1; jj >= 0; --jj)
      if (__shfl(idx, jj) == idx) lead = jj;
    const bool leader = used && lead == j;
    const unsigned long long leaders = __ballot(leader);
    const int slot = __popcll(leaders & ((1ull << j) - 1ull));
    const int my_slot = __shfl(slot, lead);
    const unsigned long long any_bad = __ballot(bad);
    const int nq = __popcll(leaders);
    if (leader && slot < kMaxRelCols) rl->qcol[slot] = idx;
    rl->tokslot[j] = (signed char)(used ? my_slot : -1);   // a slot past kMaxRelCols - 1 (at most 63) makes the row unservable
    if (j == 0) {
      rl->nq = nq;
      rl->ok = (base_ok && any_bad == 0 && nq <= rc.Q_max && nq <= kMaxRelCols) ? 1 : 0;
    }
  }
  __syncthreads();
  return rl->ok != 0;
}

// The relations' forward on the softmax statistics: per slot the mass m, the centroid column c and the centroid row cy in one
// pixel loop (block_sum: deterministic), then per relation v = (cL + 0.2 res - cR) / res * 9 in the reference's operation
// order (run.py:207-225) on the coordinate and with the roles of its kind.  Results in RelLds.
__device__ __forceinline__ void rel_forward(const LossArgs& a, const ga_image_loss_t& d, const RelCtx& rc, const float* mx,
                                            const float* gcol, float* scratch) {
  const float* sm = rc.sm2;
  const int res = a.res, npix = res * res;
  RelLds* rl = rc.st;
  for (int q = 0; q < rl->nq; ++q) {
    float v3[3] = {0.f, 0.f, 0.f};
    for (int p = threadIdx.x; p < npix; p += kThreads) {
      const float S = expf(rel_value(a, d, rc, gcol, q, p, npix) * 100.0f - mx[p]) / sm[p];
      const int i = p / res, j = p - i * res;
      v3[0] += S;
      v3[1] += S * ((float)j + 0.5f);
      v3[2] += S * ((float)i + 0.5f);
    }
    block_sum<3>(v3, scratch);
    if (threadIdx.x == 0) {
      rl->m[q] = v3[0];
      rl->c[q] = v3[1] / v3[0];
      rl->cy[q] = v3[2] / v3[0];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < rc.row->R) {
    const int r = threadIdx.x;
    const ga_relation_t& rel = rc.row->rel[r];
    const int lead = rel_lead_side(rel.kind), n_lead = lead ? rel.n_right : rel.n_left, n_other = lead ? rel.n_left : rel.n_right;
    const float* c = rel_vertical(rel.kind) ? rl->cy : rl->c;
    const float nl = (float)n_lead;
    float cL = 0.f, cR = 0.f;
    for (int k = 0; k < n_lead; ++k) cL += c[rl->tokslot[(r * 2 + lead) * GA_REL_MAX_TOKENS + k]] / nl;
    for (int k = 0; k < n_other; ++k) cR += c[rl->tokslot[(r * 2 + 1 - lead) * GA_REL_MAX_TOKENS + k]] / nl;
    const float gap = (float)(0.2 * (double)res);
    rl->cL[r] = cL;
    rl->cR[r] = cR;
    rl->v[r] = (cL + gap - cR) / (float)res * 9.0f;
  }
  __syncthreads();
}

template <bool kRel = false>
__device__ __forceinline__ void loss_forward(const LossArgs& a, const ga_image_loss_t& d, float* lds, float* __restrict__ terms,
                                             float* __restrict__ loss, const RelCtx& rc = RelCtx{}) {
  const int npix = a.res * a.res;
  float* mx = lds;
  float* sm = mx + npix;
  float* M = sm + npix;
  float* Pn = M + npix;
  float* scratch = Pn + npix;  // 16 floats
  float* W = scratch + 16;     // [npix], strict mode only
  float* gcol = W + (a.w_lds ? npix : 0);              // [T_max][npix] (kRel: [T_max + Q_max][npix])
  const int n_slots = kRel ? a.T_max + rc.Q_max : a.T_max;
  float* stage = align16(gcol + (a.use_gcol ? (size_t)n_slots * npix : 0));   // [stage_rows][Kt]
  pixel_softmax_stats<kRel>(a, d, rc, mx, sm, stage, gcol);
  __syncthreads();
  float total = 0.f;
  for (int t = 0; t < d.T; ++t) {
    const ga_token_t& tk = d.tok[t];
    const TokenStats st = token_forward(a, d, tk, mx, sm, gcol, t, M, Pn, W, scratch);
    const TokenLoss tl = token_loss(a, d, tk, st);
    total += tk.weight * tl.item;
    if (threadIdx.x == 0) {
      float* o = terms + t * GA_TERMS;
      o[0] = st.mxv;
      o[1] = st.col;
      o[2] = st.row;
      o[3] = tl.inside;
      o[4] = tl.outside;
      o[5] = tl.item;
      o[6] = tl.unscaled;
      o[7] = st.s;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = total;
  if constexpr (kRel) {
    const int R = rc.row->R;
    if (R > 0) rel_forward(a, d, rc, mx, gcol, scratch);
    if (threadIdx.x == 0) {
      float rel_total = 0.f;
      for (int r = 0; r < R; ++r) {
        const float v = rc.st->v[r], value = fmaxf(v, 0.f);
        float* o = rc.terms + r * 4;
        o[0] = value;
        o[1] = v;
        o[2] = rc.st->cL[r];
        o[3] = rc.st->cR[r];
        rel_total += value;
      }
      rc.loss[0] = rel_total;
    }
  }
}

// One image's loss into its terms rows [T_max] and loss word: rows past the descriptor's T are zero; T = 0 (an image that is
// not guided) is loss 0 without any token or softmax work, an unservable row is loss NaN.
__device__ __forceinline__ void image_loss_forward(const LossArgs& a, const ga_image_loss_t& d, float* lds,
                                                   float* __restrict__ terms, float* __restrict__ loss) {
  const bool ok = row_ok(a, d);
  const int T = ok ? d.T : 0;
  for (int e = T * GA_TERMS + (int)threadIdx.x; e < a.T_max * GA_TERMS; e += kThreads) terms[e] = 0.f;
  if (T == 0) {
    if (threadIdx.x == 0) loss[0] = ok ? 0.f : __builtin_nanf("");
    return;
  }
  loss_forward(a, d, lds, terms, loss);
}

// image_loss_forward of the *_rel_* launches: the box loss as above, then the relations.  An image without guided tokens but
// with relations runs the softmax statistics; rows past R of rel_terms are zero; an unservable row pair: both losses NaN.
__device__ __forceinline__ void image_loss_rel_forward(const LossArgs& a, const ga_image_loss_t& d, const RelCtx& rc, float* lds,
                                                       float* __restrict__ terms, float* __restrict__ loss) {
  const bool ok = rel_setup(a, d, rc, row_ok(a, d));
  const int T = ok ? d.T : 0, R = ok ? rc.row->R : 0;
  for (int e = T * GA_TERMS + (int)threadIdx.x; e < a.T_max * GA_TERMS; e += kThreads) terms[e] = 0.f;
  if ((int)threadIdx.x >= R * 4 && (int)threadIdx.x < GA_IMAGE_MAX_RELATIONS * 4) rc.terms[threadIdx.x] = 0.f;
  if (T == 0 && R == 0) {
    if (threadIdx.x == 0) loss[0] = rc.loss[0] = ok ? 0.f : __builtin_nanf("");
    return;
  }
  loss_forward<true>(a, d, lds, terms, loss, rc);
}

__global__ __launch_bounds__(kThreads) void smooth_loss_fwd_kernel(LossArgs a, float* __restrict__ terms,
                                                                   float* __restrict__ loss) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  loss_forward(a, a.img, lds, terms, loss);
}

// K2 + K3 + K4 in ONE launch (utils/ptp_utils.py:279-289 -> pipeline_guided_attention.py:217-219): every workgroup
// averages 256 (pixel, token) elements over the head-maps (aggregate.h: list order, no atomics) and stores them to A;
// the workgroup whose ticket comes last then evaluates the loss on the complete A.  Hand-off: stores drained by every
// wave, workgroup barrier, one agent-scope release + one relaxed ticket add per workgroup; the last arriver makes one
// agent-scope acquire before its plain loads of A and returns the ticket word to zero for the next launch.
// Batched (grid.y = S images): image blockIdx.y averages its own head-maps into its own A, counts on its own ticket word
// and its last arriver evaluates its own loss — the S evaluations run side by side, each one exactly the single-image work.
// kTable: that evaluation takes image blockIdx.y's descriptor row from a.table (device memory) instead of a.img.
template <typename T, bool kTable>
__global__ __launch_bounds__(kThreads) void aggregate_loss_fwd_kernel(AggArgs g, LossArgs a, int n_elem, float* __restrict__ A,
                                                                      float* __restrict__ terms, float* __restrict__ loss,
                                                                      unsigned* __restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int img = blockIdx.y;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e < n_elem) A[(size_t)img * n_elem + e] = aggregate_element<T>(g, e, n_elem, img);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int* flag = reinterpret_cast<int*>(lds);
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the fence's own wait can be dropped by the compiler: keep this one
    const unsigned old = __hip_atomic_fetch_add(ticket + img, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(ticket + img, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    flag[0] = last;
  }
  __syncthreads();
  const int last = flag[0];
  __syncthreads();   // the flag word is part of the loss's LDS image
  if (!last) return;
  if constexpr (kTable)
    image_loss_forward(a, stage_row(a.table, reinterpret_cast<ga_image_loss_t*>(lds)), lds + kRowFloats,
                       terms + (size_t)img * a.T_max * GA_TERMS, loss + img);
  else
    loss_forward(a, a.img, lds, terms + (size_t)img * a.T_max * GA_TERMS, loss + img);
}

// LDS of the *_rel_* launches in front of the loss tables: the loss row, the relation row, the relation state
constexpr int kRelFrontFloats = kRowFloats + kRelRowFloats + kRelLdsFloats;
struct RelArgs {
  const ga_image_relations_t* table;   // [images] rows in device memory
  int Q_max;
  float* terms;   // [images][GA_IMAGE_MAX_RELATIONS][4]
  float* loss;    // [images]
};
// (then sm2 [npix], then the loss tables: rel_tables)
__device__ __forceinline__ float* rel_tables(const LossArgs& a, float* lds) { return lds + kRelFrontFloats + a.res * a.res; }
__device__ __forceinline__ RelCtx rel_ctx(const RelArgs& ra, float* lds) {
  RelCtx rc;
  rc.sm2 = lds + kRelFrontFloats;
  rc.row = reinterpret_cast<const ga_image_relations_t*>(lds + kRowFloats);
  rc.st = reinterpret_cast<RelLds*>(lds + kRowFloats + kRelRowFloats);
  rc.Q_max = ra.Q_max;
  rc.terms = ra.terms ? ra.terms + (size_t)blockIdx.y * GA_IMAGE_MAX_RELATIONS * 4 : nullptr;
  rc.loss = ra.loss ? ra.loss + blockIdx.y : nullptr;
  return rc;
}

// aggregate_loss_fwd_kernel<T, true> whose last arriver also evaluates image blockIdx.y's relations (same hand-off)
template <typename T>
__global__ __launch_bounds__(kThreads) void aggregate_loss_rel_fwd_kernel(AggArgs g, LossArgs a, RelArgs ra, int n_elem,
                                                                          float* __restrict__ A, float* __restrict__ terms,
                                                                          float* __restrict__ loss,
                                                                          unsigned* __restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int img = blockIdx.y;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e < n_elem) A[(size_t)img * n_elem + e] = aggregate_element<T>(g, e, n_elem, img);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int* flag = reinterpret_cast<int*>(lds);
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned old = __hip_atomic_fetch_add(ticket + img, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(ticket + img, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    flag[0] = last;
  }
  __syncthreads();
  const int last = flag[0];
  __syncthreads();   // the flag word is part of the staged row
  if (!last) return;
  ga_image_loss_t* row = reinterpret_cast<ga_image_loss_t*>(lds);
  stage_rows_rel(a.table, ra.table, row, reinterpret_cast<ga_image_relations_t*>(lds + kRowFloats));
  image_loss_rel_forward(a, *row, rel_ctx(ra, lds), rel_tables(a, lds), terms + (size_t)img * a.T_max * GA_TERMS, loss + img);
}

template <typename T>
__device__ __attribute__((noinline)) void zero_fill(float* __restrict__ dA, T* __restrict__ dPb, int total) {
  for (int e = blockIdx.x * kThreads + threadIdx.x; e < total; e += gridDim.x * kThreads) {
    dA[e] = 0.f;
    if (dPb) dPb[e] = Traits<T>::from_f32(0.f);
  }
}

template <typename T, bool kRel = false>
__device__ __forceinline__ void loss_backward(const LossArgs& a, const ga_image_loss_t& d, float* lds, const float* __restrict__ dloss,
                                              float* __restrict__ dA, T* __restrict__ dPb, float bcast_scale, int zero_idle,
                                              const RelCtx& rc = RelCtx{}) {
  const int res = a.res, npix = res * res;
  // batched launches (grid.y = S): this workgroup's image; an image whose dloss is exactly 0 (an idle slot, or an image
  // that takes no update) gets exact zeros and none of the token work — and so does an image without guided tokens
  const int img = blockIdx.y;
  auto unguided = [&] {   // evaluated behind the dloss test, as the plain launches always did
    if constexpr (kRel) return d.T == 0 && rc.row->R == 0;
    else return d.T == 0;
  };
  if ((zero_idle && dloss[img] == 0.f) || unguided()) {
    zero_fill(dA + (size_t)img * a.img_stride, dPb ? dPb + (size_t)img * a.img_stride : nullptr, npix * a.Kt);
    return;
  }
  float* mx = lds;
  float* sm = mx + npix;
  float* M = sm + npix;
  float* Pn = M + npix;
  float* G = Pn + npix;         // dItem/dM' per pixel
  float* dot = G + npix;        // sum_k dS[p][k] S[p][k]
  float* scratch = dot + npix;  // 16 floats
  int* colmap = reinterpret_cast<int*>(scratch + 16);  // [Kt]: guided-token slot of column c, or -1
  float* dS = reinterpret_cast<float*>(colmap + ((a.Kt + 3) & ~3));  // [T_max][npix] (kRel: [T_max + Q_max][npix], and gcol)
  const int n_slots = kRel ? a.T_max + rc.Q_max : a.T_max;
  float* W = dS + (size_t)n_slots * npix;                            // [npix], strict mode only
  float* gcol = W + (a.w_lds ? npix : 0);                            // [T_max][npix]
  float* stage = align16(gcol + (a.use_gcol ? (size_t)n_slots * npix : 0));   // [stage_rows][Kt]

  pixel_softmax_stats<kRel>(a, d, rc, mx, sm, stage, gcol);
  for (int c = threadIdx.x; c < a.Kt; c += kThreads) colmap[c] = -1;
  __syncthreads();
  const int pad = a.ksize >> 1;
  const float rm1 = (float)res - 1.0f;
  for (int t = 0; t < d.T; ++t) {
    const ga_token_t& tk = d.tok[t];
    const TokenStats st = token_forward(a, d, tk, mx, sm, gcol, t, M, Pn, W, scratch);
    const TokenLoss tl = token_loss(a, d, tk, st);
    if (threadIdx.x == 0) colmap[d.first + tk.token - 1] = t;
    const float sgc = tl.dc > 0.f ? 1.f : (tl.dc < 0.f ? -1.f : 0.f);
    const float sgr = tl.dr > 0.f ? 1.f : (tl.dr < 0.f ? -1.f : 0.f);
    float gd[1] = {0.f};
    for (int p = threadIdx.x; p < npix; p += kThreads) {
      const int i = p / res, j = p - i * res;
      float g = tl.w_c * (sgc / rm1 * ((float)j + 0.5f) + 4.0f * sgr / rm1 * ((float)i + 0.5f));
      if (tk.kind == GA_TOK_BOX) {
        const bool in = inside_box(tk, res, d.shrink, i, j);
        if (d.strict)  // hinge terms: the gradient passes only where the hinge is open (Python max(min_loss, v): v > 0)
          g += in ? (st.at_most - Pn[p] > 0.f ? -2.0f * tl.w_in * W[p] : 0.f) : (Pn[p] > 0.f ? tl.w_out3 * W[p] : 0.f);
        else
          g += in ? -tl.w_in : tl.w_out3;
      }
      G[p] = g;
      gd[0] += g * Pn[p];
    }
    block_sum<1>(gd, scratch);
    for (int p = threadIdx.x; p < npix; p += kThreads) G[p] = (G[p] - gd[0]) / st.s;  // through Pn = M'/sum(M')
    __syncthreads();
    // adjoint of reflect-pad + correlation, as a gather (deterministic): dM[a][b] = sum over (i,u),(j,v)
    // with reflect(i+u-pad) == a and reflect(j+v-pad) == b of gw[u][v] * G[i][j]
    float* dSt = dS + (size_t)t * npix;
    for (int p = threadIdx.x; p < npix; p += kThreads) {
      float acc;
      if (a.smooth) {
        const int ai = p / res, bj = p - ai * res;
        acc = 0.f;
        for (int i = max(ai - pad, 0); i <= min(ai + pad, res - 1); ++i)
          for (int u = 0; u < a.ksize; ++u) {
            if (reflect_idx(i + u - pad, res) != ai) continue;
            for (int j = max(bj - pad, 0); j <= min(bj + pad, res - 1); ++j)
              for (int v = 0; v < a.ksize; ++v)
                if (reflect_idx(j + v - pad, res) == bj) acc += a.gw[u * a.ksize + v] * G[i * res + j];
          }
      } else {
        acc = G[p];
      }
      dSt[p] = tk.weight * acc;
    }
    __syncthreads();
  }
  // The relations' upstream gradient joins the box terms' dS here, in front of the one softmax Jacobian.  A relation with a
  // closed hinge (v < 0) adds nothing; when every hinge of the image is closed none of this runs and the image is exactly its
  // R = 0 self.  Slot q's column is a guided token's column: its gradient is added to that token's dS (one slot per column).
  bool rel_open = false;
  if constexpr (kRel) {
    RelLds* rl = rc.st;
    const int R = rc.row->R;
    if (R > 0) {
      rel_forward(a, d, rc, mx, gcol, scratch);
      if ((int)threadIdx.x < rl->nq) {
        const int q = threadIdx.x;
        float wx = 0.f, wy = 0.f;   // through the centroid column, through the centroid row
        for (int r = 0; r < R; ++r) {
          if (!(rl->v[r] >= 0.f)) continue;   // torch.clamp(min=0)'s backward passes where v >= 0
          const ga_relation_t& rel = rc.row->rel[r];
          const int lead = rel_lead_side(rel.kind);
          const int n_lead = lead ? rel.n_right : rel.n_left, n_other = lead ? rel.n_left : rel.n_right;
          const float coef = 9.0f / (float)res / (float)n_lead;
          float w = rel_vertical(rel.kind) ? wy : wx;   // each axis adds up in the relations' order
          for (int k = 0; k < n_lead; ++k)
            if (rl->tokslot[(r * 2 + lead) * GA_REL_MAX_TOKENS + k] == q) w += coef;
          for (int k = 0; k < n_other; ++k)
            if (rl->tokslot[(r * 2 + 1 - lead) * GA_REL_MAX_TOKENS + k] == q) w -= coef;
          if (rel_vertical(rel.kind)) wy = w;
          else wx = w;
        }
        rl->w[q] = wx;
        rl->wy[q] = wy;
        int merged = -1;
        for (int t = 0; t < d.T; ++t)
          if (d.tok[t].token - 1 == rl->qcol[q]) merged = t;   // the last one, as colmap keeps it
        rl->merged[q] = (signed char)merged;
      }
      if (threadIdx.x == 0) {
        int any = 0;
        for (int r = 0; r < R; ++r) any |= rl->v[r] >= 0.f ? 1 : 0;
        rl->any_open = any;
      }
      __syncthreads();
      rel_open = rl->any_open != 0;
      if (rel_open) {
        for (int q = 0; q < rl->nq; ++q) {
          const int merged = rl->merged[q];
          const float w = rl->w[q], c = rl->c[q], wy = rl->wy[q], cy = rl->cy[q], m = rl->m[q];
          float* dSq = dS + (size_t)(merged >= 0 ? merged : a.T_max + q) * npix;
          for (int p = threadIdx.x; p < npix; p += kThreads) {
            const int i = p / res, j = p - i * res;
            // d value / d S[p][q] through c = sum S col / m, and through cy = sum S row / m
            const float g = w * (((float)j + 0.5f) - c) / m + wy * (((float)i + 0.5f) - cy) / m;
            dSq[p] = merged >= 0 ? dSq[p] + g : g;
          }
          if (threadIdx.x == 0 && merged < 0) colmap[d.first + rl->qcol[q]] = a.T_max + q;
        }
        __syncthreads();
      }
    }
  }
  // softmax backward: dA[p][c] = 100 * S[p][c] * (dS[p][c] - sum_k dS[p][k] S[p][k]) on the text slice.  With an open relation
  // S comes from the compensated sums (smj): at a near-one-hot pixel dS - dot is dS * (1 - S), and the token-order sum's error
  // in S was 5e-6 of the gradient's maximum on the BOS-heavy fixture map, four times the plugin's own float32 error.
  const float* smj = sm;
  if constexpr (kRel)
    if (rel_open) smj = rc.sm2;
  for (int p = threadIdx.x; p < npix; p += kThreads) {
    float dd = 0.f;
    for (int t = 0; t < d.T; ++t) dd += dS[(size_t)t * npix + p] * (expf(guided_value(a, d, gcol, t, p, npix) * 100.0f - mx[p]) / smj[p]);
    if constexpr (kRel)
      if (rel_open)
        for (int q = 0; q < rc.st->nq; ++q)
          if (rc.st->merged[q] < 0)
            dd += dS[(size_t)(a.T_max + q) * npix + p] * (expf(rel_value(a, d, rc, gcol, q, p, npix) * 100.0f - mx[p]) / smj[p]);
    dot[p] = dd;
  }
  __syncthreads();
  // every workgroup has derived the same per-pixel tables (the token work above is 3 x 256 pixels: repeating it costs
  // less than any hand-off); the element-wise tail over the (pixel, token) grid is split between them
  const float dl = dloss ? dloss[img] : 1.0f;
  const int total = npix * a.Kt;
  for (int e0 = blockIdx.x * kThreads + threadIdx.x; e0 < total; e0 += 4 * gridDim.x * kThreads) {
    float av[4];   // four loads in flight per thread, then the math
#pragma unroll
    for (int u = 0; u < 4; ++u) av[u] = image_A(a)[min(e0 + u * (int)(gridDim.x * kThreads), total - 1)];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * (int)(gridDim.x * kThreads);
      if (e >= total) break;
      const int p = e / a.Kt, c = e - p * a.Kt;
      float g = 0.f;
      if (c >= d.first && c < d.last) {
        const float S = expf(av[u] * 100.0f - mx[p]) / smj[p];
        const int t = colmap[c];
        g = dl * 100.0f * S * ((t >= 0 ? dS[(size_t)t * npix + p] : 0.f) - dot[p]);
      }
      dA[(size_t)img * a.img_stride + e] = g;
      if (dPb) dPb[(size_t)img * a.img_stride + e] = Traits<T>::from_f32(g * bcast_scale);
    }
  }
}

template <typename T, bool kTable>
__global__ __launch_bounds__(kThreads) void smooth_loss_bwd_kernel(LossArgs a, const float* __restrict__ dloss,
                                                                   float* __restrict__ dA, T* __restrict__ dPb,
                                                                   float bcast_scale, int zero_idle) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if constexpr (kTable) {
    const ga_image_loss_t& d = stage_row(a.table, reinterpret_cast<ga_image_loss_t*>(lds));
    if (!row_ok(a, d)) {   // an unservable row: zeros, as for an image without guided tokens
      zero_fill(dA + (size_t)blockIdx.y * a.img_stride, dPb ? dPb + (size_t)blockIdx.y * a.img_stride : nullptr,
                a.res * a.res * a.Kt);
      return;
    }
    loss_backward<T>(a, d, lds + kRowFloats, dloss, dA, dPb, bcast_scale, zero_idle);
  } else {
    loss_backward<T>(a, a.img, lds, dloss, dA, dPb, bcast_scale, zero_idle);
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void smooth_loss_rel_bwd_kernel(LossArgs a, RelArgs ra, const float* __restrict__ dloss,
                                                                       float* __restrict__ dA, T* __restrict__ dPb,
                                                                       float bcast_scale) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  ga_image_loss_t* row = reinterpret_cast<ga_image_loss_t*>(lds);
  stage_rows_rel(a.table, ra.table, row, reinterpret_cast<ga_image_relations_t*>(lds + kRowFloats));
  const RelCtx rc = rel_ctx(ra, lds);
  if (!rel_setup(a, *row, rc, row_ok(a, *row))) {   // an unservable row pair: zeros
    zero_fill(dA + (size_t)blockIdx.y * a.img_stride, dPb ? dPb + (size_t)blockIdx.y * a.img_stride : nullptr,
              a.res * a.res * a.Kt);
    return;
  }
  loss_backward<T, true>(a, *row, rel_tables(a, lds), dloss, dA, dPb, bcast_scale, 1, rc);
}

size_t fwd_lds(int npix, int strict) { return sizeof(float) * ((4 + (strict ? 1 : 0)) * (size_t)npix + 16); }
size_t bwd_lds(int npix, int Kt, int T, int strict) {
  return sizeof(float) * ((6 + (strict ? 1 : 0)) * (size_t)npix + 16 + ((Kt + 3) & ~3) + (size_t)T * npix);
}
constexpr size_t kLdsBudget = 150 * 1024;
// rows of A staged per pass: as many as fit beside the kernel's tables, at most one per thread, a multiple of 4
int choose_stage_rows(size_t base_lds, int npix, int Kt, const float* A) {
  if ((reinterpret_cast<uintptr_t>(A) & 15) != 0) return 0;
  base_lds += 16;   // the staging area starts on a 16-byte boundary
  for (int rows = kThreads; rows >= 32; rows >>= 1) {
    const int r = rows < npix ? rows : ((npix + 3) & ~3);
    if (base_lds + sizeof(float) * (size_t)r * Kt <= kLdsBudget) return r;
  }
  return 0;
}

// The shape checks of the launches, shared with the plan query (ga_loss_lds_plan answers what the launch would).
int check_call_shape(int res, int Kt, int T_max) {
  return (res < 2 || res > 64 || Kt < 2 || T_max < 1 || T_max > kMaxTok) ? GA_ERR_SHAPE : GA_OK;
}
int check_images(int images) { return (images < 1 || images > GA_MAX_IMAGES) ? GA_ERR_SHAPE : GA_OK; }
int check_table_shape(int T_max, int res) { return (long long)T_max * res * res > 24576 ? GA_ERR_SHAPE : GA_OK; }
int check_rel_shape(int Q_max, int T_max, int res) {
  if (Q_max < 0 || Q_max > kMaxRelCols) return GA_ERR_SHAPE;
  if ((long long)(T_max + Q_max) * res * res > 24576) return GA_ERR_SHAPE;
  return GA_OK;
}

// The LDS plan of one launch.  The fixed tables first (forward: fwd_lds, backward: bwd_lds, the relation launches' sm2), the
// guided columns when they fit into half the budget with them, then the staging area with what is left; in front of it all
// the staged descriptor row(s) of the table / relation launches.  `A_batched`: a batched A ([S][npix][Kt]) is staged only when
// every image's slice stays 16-byte aligned.  Every launch takes its plan from here, and so does ga_loss_lds_plan.
struct LdsPlan {
  int use_gcol, stage_rows;
  size_t lds;
};
int loss_lds_plan(LdsPlan& pl, bool backward, bool table, bool rel, int images, int res, int Kt, int T_max, int Q_max, int w_lds,
                  const float* A) {
  const int npix = res * res, slots = T_max + (rel ? Q_max : 0);
  size_t lds = (backward ? bwd_lds(npix, Kt, slots, w_lds) : fwd_lds(npix, w_lds)) + (rel ? sizeof(float) * npix : 0);
  if (lds > kLdsBudget) return GA_ERR_SHAPE;
  pl.use_gcol = lds + sizeof(float) * (size_t)slots * npix <= kLdsBudget / 2 ? 1 : 0;
  if (pl.use_gcol) lds += sizeof(float) * (size_t)slots * npix;
  const bool A_batched = images > 1;
  pl.stage_rows = (A_batched && ((size_t)npix * Kt) % 4 != 0) ? 0 : choose_stage_rows(lds, npix, Kt, A);
  lds += sizeof(float) * (size_t)pl.stage_rows * Kt + 16;
  if (rel)
    lds += sizeof(float) * kRelFrontFloats;
  else if (table)
    lds += sizeof(float) * kRowFloats;
  pl.lds = lds;
  return GA_OK;
}

// the call-level arguments: map, shape, token capacity, smoothing (every image of a launch shares the Gaussian weights)
int fill_call_args(LossArgs& a, const float* A, int res, int Kt, int T_max, const ga_loss_params_t* hp) {
  if (!A || !hp) return GA_ERR_NULL;
  if (check_call_shape(res, Kt, T_max) != GA_OK) return GA_ERR_SHAPE;
  if (hp->smooth && (hp->ksize < 1 || hp->ksize > kMaxK || (hp->ksize & 1) == 0 || hp->ksize / 2 >= res))
    return GA_ERR_SHAPE;
  a.A = A;
  a.img_stride = (long long)res * res * Kt;
  a.res = res;
  a.Kt = Kt;
  a.T_max = T_max;
  a.ksize = hp->smooth ? hp->ksize : 1;
  a.smooth = hp->smooth ? 1 : 0;
  a.w_lds = 0;
  a.table = nullptr;
  a.img = ga_image_loss_t{};
  if (a.smooth) {
    int rc = ga_gaussian_weights(hp->ksize, hp->sigma, a.gw);
    if (rc != GA_OK) return rc;
  }
  return GA_OK;
}

// the argument form: one descriptor for every image of the launch, checked here
int fill_args(LossArgs& a, const float* A, int res, int Kt, int first, int last, const ga_token_t* tokens, int T,
              const ga_loss_params_t* hp) {
  if (!A || !tokens || !hp) return GA_ERR_NULL;
  int rc = fill_call_args(a, A, res, Kt, T, hp);
  if (rc != GA_OK) return rc;
  if (first < 0 || last > Kt || last - first < 1) return GA_ERR_SHAPE;
  ga_image_loss_t& d = a.img;
  for (int t = 0; t < T; ++t) {
    const int col = first + tokens[t].token - 1;
    if (col < first || col >= last) return GA_ERR_SHAPE;
    if (tokens[t].kind != GA_TOK_BOX && tokens[t].kind != GA_TOK_COOR) return GA_ERR_UNSUPPORTED;
    d.tok[t] = tokens[t];
  }
  d.first = first;
  d.last = last;
  d.T = T;
  d.strict = hp->strict ? 1 : 0;
  d.inside_scale = hp->inside_scale;
  d.outside_scale = hp->outside_scale;
  d.center_weight = hp->center_weight;
  d.shrink = hp->shrink;
  a.w_lds = d.strict;
  return GA_OK;
}

// the table form: the rows live in device memory (row_ok screens them in the kernels)
int fill_table_args(LossArgs& a, const float* A, int images, int res, int Kt, const ga_image_loss_t* table, int T_max,
                    const ga_loss_params_t* shared_hp) {
  if (!table) return GA_ERR_NULL;
  if (check_images(images) != GA_OK) return GA_ERR_SHAPE;
  int rc = fill_call_args(a, A, res, Kt, T_max, shared_hp);
  if (rc != GA_OK) return rc;
  if (check_table_shape(T_max, res) != GA_OK) return GA_ERR_SHAPE;
  a.table = table;
  a.w_lds = 1;   // any row may be strict
  return GA_OK;
}

}  // namespace

extern "C" int ga_gaussian_weights(int ksize, float sigma, float* w) {
  if (!w) return GA_ERR_NULL;
  if (ksize < 1 || ksize > kMaxK || !(sigma > 0.f)) return GA_ERR_SHAPE;
  // utils/gaussian_smoothing.py:30-43 in fp32: per dimension 1/(std*sqrt(2*pi)) * exp(-((x-mean)/(2*std))^2),
  // product over the two dimensions, then divided by the sum
  float g1[kMaxK];
  const float mean = (float)((ksize - 1) / 2.0);
  const float norm = (float)(1.0 / ((double)sigma * 2.5066282746310002));
  for (int i = 0; i < ksize; ++i) {
    const float z = ((float)i - mean) / (2.0f * sigma);
    g1[i] = norm * expf(-(z * z));
  }
  float sum = 0.f;
  for (int i = 0; i < ksize; ++i)
    for (int j = 0; j < ksize; ++j) {
      w[i * ksize + j] = g1[i] * g1[j];
      sum += w[i * ksize + j];
    }
  for (int i = 0; i < ksize * ksize; ++i) w[i] /= sum;
  return GA_OK;
}

extern "C" int ga_smooth_loss_fwd(const float* A, int res, int Kt, int first, int last, const ga_token_t* tokens, int T,
                                  const ga_loss_params_t* hp, float* terms, float* loss, ga_stream_t stream) {
  if (!terms || !loss) return GA_ERR_NULL;
  LossArgs a;
  int rc = fill_args(a, A, res, Kt, first, last, tokens, T, hp);
  if (rc != GA_OK) return rc;
  LdsPlan pl;
  rc = loss_lds_plan(pl, false, false, false, 1, res, Kt, T, 0, a.w_lds, A);
  if (rc != GA_OK) return rc;
  a.use_gcol = pl.use_gcol;
  a.stage_rows = pl.stage_rows;
  if (set_dyn_lds(smooth_loss_fwd_kernel, pl.lds) != GA_OK) return GA_ERR_LAUNCH;
  hipLaunchKernelGGL(smooth_loss_fwd_kernel, dim3(1), dim3(kThreads), pl.lds, static_cast<hipStream_t>(stream), a, terms,
                     loss);
  return check_launch();
}

// `ra` (the *_rel_* entries): the relation table; its Q_max slots sit behind the T_max token slots of gcol and dS
template <typename T>
static int launch_loss_bwd(const LossArgs& a, const RelArgs* ra, const float* dloss, float* dA, void* dPb, float bs, size_t lds,
                           int images, int zero_idle, hipStream_t s) {
  // up to 16 workgroups per image, at least 4 elements of the tail per thread
  const int total = a.res * a.res * a.Kt;
  const int wgs = max(1, min(16, total / (4 * kThreads)));
  if (ra) {
    auto k = smooth_loss_rel_bwd_kernel<T>;
    if (set_dyn_lds(k, lds) != GA_OK) return GA_ERR_LAUNCH;
    hipLaunchKernelGGL(k, dim3(wgs, images), dim3(kThreads), lds, s, a, *ra, dloss, dA, (T*)dPb, bs);
    return check_launch();
  }
  auto k = a.table ? smooth_loss_bwd_kernel<T, true> : smooth_loss_bwd_kernel<T, false>;
  if (set_dyn_lds(k, lds) != GA_OK) return GA_ERR_LAUNCH;
  hipLaunchKernelGGL(k, dim3(wgs, images), dim3(kThreads), lds, s, a, dloss, dA, (T*)dPb, bs, zero_idle);
  return check_launch();
}

static int loss_bwd(LossArgs& a, int images, int zero_idle, const float* dloss, float* dA, void* dP_bcast, float bcast_scale,
                    int dtype, ga_stream_t stream, const RelArgs* ra = nullptr) {
  LdsPlan pl;
  int rc = loss_lds_plan(pl, true, a.table != nullptr, ra != nullptr, images, a.res, a.Kt, a.T_max, ra ? ra->Q_max : 0, a.w_lds, a.A);
  if (rc != GA_OK) return rc;
  a.use_gcol = pl.use_gcol;
  a.stage_rows = pl.stage_rows;
  const size_t lds = pl.lds;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case GA_F16:
      return launch_loss_bwd<_Float16>(a, ra, dloss, dA, dP_bcast, bcast_scale, lds, images, zero_idle, s);
    case GA_BF16:
      return launch_loss_bwd<bf16_t>(a, ra, dloss, dA, dP_bcast, bcast_scale, lds, images, zero_idle, s);
    case GA_F32:
      return launch_loss_bwd<float>(a, ra, dloss, dA, dP_bcast, bcast_scale, lds, images, zero_idle, s);
    default:
      return GA_ERR_DTYPE;
  }
}

extern "C" int ga_smooth_loss_bwd(const float* A, int res, int Kt, int first, int last, const ga_token_t* tokens, int T,
                                  const ga_loss_params_t* hp, const float* dloss, float* dA, void* dP_bcast,
                                  float bcast_scale, int dtype, ga_stream_t stream) {
  if (!dA) return GA_ERR_NULL;
  LossArgs a;
  int rc = fill_args(a, A, res, Kt, first, last, tokens, T, hp);
  if (rc != GA_OK) return rc;
  return loss_bwd(a, 1, 0, dloss, dA, dP_bcast, bcast_scale, dtype, stream);
}

extern "C" int ga_smooth_loss_bwd_batched(const float* A, int images, int res, int Kt, int first, int last,
                                          const ga_token_t* tokens, int T, const ga_loss_params_t* hp, const float* dloss,
                                          float* dA, void* dP_bcast, float bcast_scale, int dtype, ga_stream_t stream) {
  if (!dloss || !dA) return GA_ERR_NULL;
  if (check_images(images) != GA_OK) return GA_ERR_SHAPE;
  LossArgs a;
  int rc = fill_args(a, A, res, Kt, first, last, tokens, T, hp);
  if (rc != GA_OK) return rc;
  return loss_bwd(a, images, 1, dloss, dA, dP_bcast, bcast_scale, dtype, stream);
}

extern "C" int ga_smooth_loss_bwd_images(const float* A, int images, int res, int Kt, const ga_image_loss_t* table, int T_max,
                                         const ga_loss_params_t* shared_hp, const float* dloss, float* dA, void* dP_bcast,
                                         float bcast_scale, int dtype, ga_stream_t stream) {
  if (!dloss || !dA) return GA_ERR_NULL;
  LossArgs a;
  int rc = fill_table_args(a, A, images, res, Kt, table, T_max, shared_hp);
  if (rc != GA_OK) return rc;
  return loss_bwd(a, images, 1, dloss, dA, dP_bcast, bcast_scale, dtype, stream);
}

template <typename T>
static int launch_aggregate_loss(const AggArgs& g, const LossArgs& a, const RelArgs* ra, int n_elem, float* A, float* terms,
                                 float* loss, unsigned* ticket, size_t lds, int images, hipStream_t s) {
  if (ra) {
    auto k = aggregate_loss_rel_fwd_kernel<T>;
    if (set_dyn_lds(k, lds) != GA_OK) return GA_ERR_LAUNCH;
    hipLaunchKernelGGL(k, dim3((n_elem + kThreads - 1) / kThreads, images), dim3(kThreads), lds, s, g, a, *ra, n_elem, A, terms,
                       loss, ticket);
    return check_launch();
  }
  auto k = a.table ? aggregate_loss_fwd_kernel<T, true> : aggregate_loss_fwd_kernel<T, false>;
  if (set_dyn_lds(k, lds) != GA_OK) return GA_ERR_LAUNCH;
  hipLaunchKernelGGL(k, dim3((n_elem + kThreads - 1) / kThreads, images), dim3(kThreads), lds, s, g, a, n_elem, A, terms,
                     loss, ticket);
  return check_launch();
}

// `a`: filled by fill_args (one descriptor) or fill_table_args (a row per image)
static int aggregate_loss(const void* const* maps, const int* heads, int n_maps, int images, LossArgs& a, float* A,
                          float* terms, float* loss, unsigned* ticket, int dtype, ga_stream_t stream,
                          const RelArgs* ra = nullptr) {
  if (!terms || !loss || !ticket) return GA_ERR_NULL;
  AggArgs g;
  int rc = fill_agg_args(g, maps, heads, n_maps);
  if (rc != GA_OK) return rc;
  for (int i = 0; i < n_maps; ++i)   // heads[i] counts every image's head-maps of tensor i: S x (heads per image)
    if (heads[i] % images != 0) return GA_ERR_SHAPE;
  g.total_heads /= images;
  for (int i = 0; i < n_maps; ++i) g.heads[i] /= images;
  const int res = a.res, Kt = a.Kt;
  LdsPlan pl;
  rc = loss_lds_plan(pl, false, a.table != nullptr, ra != nullptr, images, res, Kt, a.T_max, ra ? ra->Q_max : 0, a.w_lds, A);
  if (rc != GA_OK) return rc;
  a.use_gcol = pl.use_gcol;
  a.stage_rows = pl.stage_rows;
  const size_t lds = pl.lds;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n_elem = res * res * Kt;
  switch (dtype) {
    case GA_F16:
      return launch_aggregate_loss<_Float16>(g, a, ra, n_elem, A, terms, loss, ticket, lds, images, s);
    case GA_BF16:
      return launch_aggregate_loss<bf16_t>(g, a, ra, n_elem, A, terms, loss, ticket, lds, images, s);
    case GA_F32:
      return launch_aggregate_loss<float>(g, a, ra, n_elem, A, terms, loss, ticket, lds, images, s);
    default:
      return GA_ERR_DTYPE;
  }
}

extern "C" int ga_aggregate_loss_fwd(const void* const* maps, const int* heads, int n_maps, int res, int Kt, int first,
                                     int last, const ga_token_t* tokens, int T, const ga_loss_params_t* hp, float* A,
                                     float* terms, float* loss, unsigned* ticket, int dtype, ga_stream_t stream) {
  LossArgs a;
  int rc = fill_args(a, A, res, Kt, first, last, tokens, T, hp);
  if (rc != GA_OK) return rc;
  return aggregate_loss(maps, heads, n_maps, 1, a, A, terms, loss, ticket, dtype, stream);
}

extern "C" int ga_aggregate_loss_fwd_batched(const void* const* maps, const int* heads, int n_maps, int images, int res,
                                             int Kt, int first, int last, const ga_token_t* tokens, int T,
                                             const ga_loss_params_t* hp, float* A, float* terms, float* loss,
                                             unsigned* tickets, int dtype, ga_stream_t stream) {
  if (check_images(images) != GA_OK) return GA_ERR_SHAPE;
  LossArgs a;
  int rc = fill_args(a, A, res, Kt, first, last, tokens, T, hp);
  if (rc != GA_OK) return rc;
  return aggregate_loss(maps, heads, n_maps, images, a, A, terms, loss, tickets, dtype, stream);
}

extern "C" int ga_aggregate_loss_fwd_images(const void* const* maps, const int* heads, int n_maps, int images, int res, int Kt,
                                            const ga_image_loss_t* table, int T_max, const ga_loss_params_t* shared_hp,
                                            float* A, float* terms, float* loss, unsigned* tickets, int dtype,
                                            ga_stream_t stream) {
  LossArgs a;
  int rc = fill_table_args(a, A, images, res, Kt, table, T_max, shared_hp);
  if (rc != GA_OK) return rc;
  return aggregate_loss(maps, heads, n_maps, images, a, A, terms, loss, tickets, dtype, stream);
}

// the relation table's host checks (the kernels screen the rows: rel_setup)
static int check_rel_args(const ga_image_relations_t* rel_table, int Q_max, int T_max, int res) {
  if (!rel_table) return GA_ERR_NULL;
  return check_rel_shape(Q_max, T_max, res);
}

extern "C" int ga_aggregate_loss_rel_fwd_images(const void* const* maps, const int* heads, int n_maps, int images, int res, int Kt,
                                                const ga_image_loss_t* table, int T_max, const ga_image_relations_t* rel_table,
                                                int Q_max, const ga_loss_params_t* shared_hp, float* A, float* terms, float* loss,
                                                float* rel_terms, float* rel_loss, unsigned* tickets, int dtype,
                                                ga_stream_t stream) {
  if (!rel_terms || !rel_loss) return GA_ERR_NULL;
  LossArgs a;
  int rc = fill_table_args(a, A, images, res, Kt, table, T_max, shared_hp);
  if (rc != GA_OK) return rc;
  rc = check_rel_args(rel_table, Q_max, T_max, res);
  if (rc != GA_OK) return rc;
  const RelArgs ra{rel_table, Q_max, rel_terms, rel_loss};
  return aggregate_loss(maps, heads, n_maps, images, a, A, terms, loss, tickets, dtype, stream, &ra);
}

extern "C" int ga_smooth_loss_rel_bwd_images(const float* A, int images, int res, int Kt, const ga_image_loss_t* table, int T_max,
                                             const ga_image_relations_t* rel_table, int Q_max, const ga_loss_params_t* shared_hp,
                                             const float* dloss, float* dA, void* dP_bcast, float bcast_scale, int dtype,
                                             ga_stream_t stream) {
  if (!dloss || !dA) return GA_ERR_NULL;
  LossArgs a;
  int rc = fill_table_args(a, A, images, res, Kt, table, T_max, shared_hp);
  if (rc != GA_OK) return rc;
  rc = check_rel_args(rel_table, Q_max, T_max, res);
  if (rc != GA_OK) return rc;
  const RelArgs ra{rel_table, Q_max, nullptr, nullptr};
  return loss_bwd(a, images, 1, dloss, dA, dP_bcast, bcast_scale, dtype, stream, &ra);
}

extern "C" int ga_loss_lds_plan(int kind, int table_form, int relations, int images, int res, int Kt, int slots, int Q_max,
                                int strict, const void* A, int* use_gcol, int* stage_rows, long long* lds_bytes) {
  if (!A || !use_gcol || !stage_rows || !lds_bytes) return GA_ERR_NULL;
  if (kind != GA_LOSS_PLAN_FWD && kind != GA_LOSS_PLAN_AGG_FWD && kind != GA_LOSS_PLAN_BWD) return GA_ERR_UNSUPPORTED;
  if ((kind == GA_LOSS_PLAN_FWD && (table_form || images != 1)) || (relations && !table_form)) return GA_ERR_UNSUPPORTED;
  // the order of the launches' own checks: images, the call's shape, the table's and the relation table's capacity, the LDS
  if (check_images(images) != GA_OK || check_call_shape(res, Kt, slots) != GA_OK) return GA_ERR_SHAPE;
  if (table_form && check_table_shape(slots, res) != GA_OK) return GA_ERR_SHAPE;
  if (relations && check_rel_shape(Q_max, slots, res) != GA_OK) return GA_ERR_SHAPE;
  LdsPlan pl;
  const int w_lds = table_form ? 1 : (strict ? 1 : 0);   // fill_table_args / fill_args
  int rc = loss_lds_plan(pl, kind == GA_LOSS_PLAN_BWD, table_form != 0, relations != 0, images, res, Kt, slots, Q_max, w_lds,
                         static_cast<const float*>(A));
  if (rc != GA_OK) return rc;
  *use_gcol = pl.use_gcol;
  *stage_rows = pl.stage_rows;
  *lds_bytes = (long long)pl.lds;
  return GA_OK;
}
