// Detection error breakdown for the eval path (extends eval_vit.py:191-292; the reference's
// "detailed error analysis" future-work item). Two kernels behind ivit_det_errors:
//
// det_errors_kernel, one workgroup per sample:
//   A  best GT per prediction exactly as det_match_kernel at thr_fg (first index of the row max
//      under strict >, f32 compare), first[g] = first qualifying prediction of GT g (LDS
//      atomicMin), floc[g] = first LOC prediction of GT g, cmax[g] = column maximum (LDS integer
//      atomicMax on the bits of the non-negative f32: the bit pattern orders like the value);
//   B  category of every prediction (TP / DUP / LOC / BKG), the fix_loc promotion flag, the
//      range bin, the four TP error terms in f64, counts and the intention confusion matrix
//      through LDS integer atomics;
//   C  status of every GT (MATCHED / MISSED_NEAR / MISSED_NONE) and its range bin;
//   D  the f64 error sums per (bin, term): each thread adds its predictions in index order, then
//      a wave butterfly and the four wave partials in wave order — a fixed order, no
//      floating-point atomics, so two runs give the same bits.
// det_errors_ap_kernel, one workgroup per (sample, variant): the keep- and TP-mask of the variant
//   from the category byte, then det_match_kernel's phases B and C over the kept predictions
//   (rank from a block scan of the keep-mask).
#include "ivit_common.h"

namespace {

constexpr int MT = 256;
constexpr int MAX_GT = 4096;
constexpr int MAX_BINS = 8;
constexpr int NI = 8;          // intention classes of the confusion matrix
constexpr int NVAR = 5;        // base, no_dup, no_bkg, fix_loc, no_miss
constexpr int K_TALLY = 12;    // TP DUP LOC BKG MISSED_NEAR MISSED_NONE GT ate ase aoe aoe_pi intent_skipped
constexpr int NONE = 0x7fffffff;

enum : unsigned char { CAT_TP = 0, CAT_DUP = 1, CAT_LOC = 2, CAT_BKG = 3 };
enum : unsigned char { GT_MATCHED = 0, GT_MISSED_NEAR = 1, GT_MISSED_NONE = 2 };
constexpr unsigned char AUX_PROMOTE = 8;  // aux byte: bits 0..2 range bin, bit 3 fix_loc promotion

struct Edges {
  float e[MAX_BINS - 1];
  int n;
};

// inclusive block scan (sum or max) of one value per thread; every thread gets its prefix
template <bool MAX>
IVIT_DEV float block_scan(float v, float* sh) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float u = __shfl_up(v, o, 64);
    if (lane >= o) v = MAX ? fmaxf(v, u) : v + u;
  }
  if (lane == 63) sh[w] = v;
  __syncthreads();
  float c = MAX ? -INFINITY : 0.f;
  for (int i = 0; i < w; ++i) c = MAX ? fmaxf(c, sh[i]) : c + sh[i];
  __syncthreads();
  return MAX ? fmaxf(v, c) : v + c;
}

// bin b holds edges[b-1] <= r < edges[b], r = sqrt(cx^2 + cy^2) in f64
IVIT_DEV int range_bin(const float* box, const Edges& ed) {
  const double x = (double)box[0], y = (double)box[1];
  const double r = sqrt(x * x + y * y);
  int b = 0;
  for (int i = 0; i < ed.n; ++i) b += r >= (double)ed.e[i];
  return b;
}

__global__ __launch_bounds__(MT) void det_errors_kernel(
    const float* __restrict__ iou, const long* __restrict__ iou_off, const int* __restrict__ npred,
    const int* __restrict__ ngt, const long* __restrict__ pred_off, const long* __restrict__ gt_off,
    const float* __restrict__ pbox, const float* __restrict__ gbox, const int* __restrict__ pint,
    const int* __restrict__ gint, float thr_fg, float thr_bg, Edges ed, unsigned char* __restrict__ cat_out,
    unsigned char* __restrict__ gts_out, int* __restrict__ best_out, double* __restrict__ err_out,
    double* __restrict__ tally, int* __restrict__ conf_out, unsigned char* __restrict__ aux_ws,
    int* __restrict__ nmatched_ws) {
  __shared__ int first[MAX_GT];
  __shared__ int floc[MAX_GT];
  __shared__ unsigned cmax[MAX_GT];
  __shared__ int cnt[MAX_BINS][8];  // 4 categories, 2 missed kinds, GT, intent_skipped
  __shared__ int conf[MAX_BINS * NI * NI];
  __shared__ double red[4][MT / 64];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int P = npred[s], G = ngt[s], nb = ed.n + 1;
  const float* M = iou + iou_off[s];
  const long po = pred_off[s], go = gt_off[s];
  unsigned char* cat = cat_out + po;
  unsigned char* aux = aux_ws + po;
  int* best = best_out + po;
  double* err = err_out + 4 * po;
  for (int g = tid; g < G; g += MT) {
    first[g] = NONE;
    floc[g] = NONE;
    cmax[g] = 0u;
  }
  for (int i = tid; i < MAX_BINS * 8; i += MT) (&cnt[0][0])[i] = 0;
  for (int i = tid; i < MAX_BINS * NI * NI; i += MT) conf[i] = 0;
  __syncthreads();
  // A: best GT (first max), provisional category (TP = qualifies), firsts and column maxima
  for (int p = tid; p < P; p += MT) {
    int bg = -1;
    unsigned char c = CAT_BKG;  // no GT: every prediction is background
    if (G > 0) {
      const float* row = M + (long)p * G;
      float bv = row[0];
      bg = 0;
      if (bv > 0.f) atomicMax(&cmax[0], __float_as_uint(bv));
      for (int g = 1; g < G; ++g) {
        const float v = row[g];
        if (v > 0.f) atomicMax(&cmax[g], __float_as_uint(v));  // NaN and negatives never enter
        if (v > bv) { bv = v; bg = g; }  // strict: first index on ties; NaN never wins
      }
      if (bv >= thr_fg) {
        c = CAT_TP;
        atomicMin(&first[bg], p);
      } else if (bv >= thr_bg) {
        c = CAT_LOC;
        atomicMin(&floc[bg], p);
      }
    }
    best[p] = bg;
    cat[p] = c;
  }
  __syncthreads();
  // B: final category, promotion flag, bin, TP errors, counts, confusion (same p -> thread map as A)
  for (int p = tid; p < P; p += MT) {
    const int bg = best[p];
    unsigned char c = cat[p];
    if (c == CAT_TP && first[bg] != p) c = CAT_DUP;
    const bool promote = c == CAT_LOC && first[bg] == NONE && floc[bg] == p;
    const float* pb = pbox + 5 * (po + p);
    double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;
    int b;
    if (c == CAT_TP) {
      const float* gb = gbox + 5 * (go + bg);
      b = range_bin(gb, ed);
      const double dx = (double)pb[0] - (double)gb[0], dy = (double)pb[1] - (double)gb[1];
      e0 = sqrt(dx * dx + dy * dy);
      const double w0 = pb[2], l0 = pb[3], w1 = gb[2], l1 = gb[3];
      const double in = fmin(w0, w1) * fmin(l0, l1);
      e1 = 1.0 - in / (w0 * l0 + w1 * l1 - in);
      const double dyaw = (double)pb[4] - (double)gb[4];
      e2 = fabs(remainder(dyaw, 6.283185307179586));
      e3 = fabs(remainder(dyaw, 3.141592653589793));
      const int gi = gint[go + bg], pi = pint[po + p];
      if ((unsigned)gi < (unsigned)NI && (unsigned)pi < (unsigned)NI) atomicAdd(&conf[(b * NI + gi) * NI + pi], 1);
      else atomicAdd(&cnt[b][7], 1);
    } else {
      b = range_bin(pb, ed);
    }
    atomicAdd(&cnt[b][c], 1);
    cat[p] = c;
    aux[p] = (unsigned char)(b | (promote ? AUX_PROMOTE : 0));
    err[4 * p + 0] = e0;
    err[4 * p + 1] = e1;
    err[4 * p + 2] = e2;
    err[4 * p + 3] = e3;
  }
  // C: GT status
  for (int g = tid; g < G; g += MT) {
    const int b = range_bin(gbox + 5 * (go + g), ed);
    unsigned char st = GT_MATCHED;
    if (first[g] == NONE) {
      st = (P > 0 && __uint_as_float(cmax[g]) >= thr_bg) ? GT_MISSED_NEAR : GT_MISSED_NONE;
      atomicAdd(&cnt[b][3 + st], 1);
    }
    atomicAdd(&cnt[b][6], 1);
    gts_out[go + g] = st;
  }
  __syncthreads();
  // D: error sums per (bin, term) in a fixed order; thread t re-reads what it wrote in B
  double* trow = tally + (long)s * nb * K_TALLY;
  for (int b = 0; b < nb; ++b) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (cnt[b][CAT_TP] > 0) {  // block-uniform
      for (int p = tid; p < P; p += MT) {
        if (cat[p] == CAT_TP && (aux[p] & 7) == b) {
          a0 += err[4 * p + 0];
          a1 += err[4 * p + 1];
          a2 += err[4 * p + 2];
          a3 += err[4 * p + 3];
        }
      }
      for (int o = 32; o >= 1; o >>= 1) {
        a0 += __shfl_xor(a0, o, 64);
        a1 += __shfl_xor(a1, o, 64);
        a2 += __shfl_xor(a2, o, 64);
        a3 += __shfl_xor(a3, o, 64);
      }
      if ((tid & 63) == 0) {
        red[0][tid >> 6] = a0;
        red[1][tid >> 6] = a1;
        red[2][tid >> 6] = a2;
        red[3][tid >> 6] = a3;
      }
      __syncthreads();
    }
    if (tid < 4) {
      double a = 0.0;
      if (cnt[b][CAT_TP] > 0)
        for (int i = 0; i < MT / 64; ++i) a += red[tid][i];
      trow[b * K_TALLY + 7 + tid] = a;
    } else if (tid >= 64 && tid < 64 + 7) {
      trow[b * K_TALLY + (tid - 64)] = (double)cnt[b][tid - 64];
    } else if (tid == 64 + 7) {
      trow[b * K_TALLY + 11] = (double)cnt[b][7];
    }
    __syncthreads();  // red is reused by the next bin
  }
  int* crow = conf_out + (long)s * nb * NI * NI;
  for (int i = tid; i < nb * NI * NI; i += MT) crow[i] = conf[i];
  if (tid == 0) {
    int m = 0;
    for (int b = 0; b < nb; ++b) m += cnt[b][CAT_TP];
    nmatched_ws[s] = m;
  }
}

// keep- and TP-mask of one variant
IVIT_DEV void variant_masks(int v, unsigned char c, unsigned char a, bool& keep, bool& tp) {
  tp = c == CAT_TP;
  keep = true;
  if (v == 1) keep = c != CAT_DUP;
  else if (v == 2) keep = c != CAT_BKG;
  else if (v == 3 && c == CAT_LOC) keep = tp = (a & AUX_PROMOTE) != 0;
}

__global__ __launch_bounds__(MT) void det_errors_ap_kernel(const int* __restrict__ npred, const int* __restrict__ ngt,
                                                           const long* __restrict__ pred_off, long ptot,
                                                           const unsigned char* __restrict__ cat_in,
                                                           const unsigned char* __restrict__ aux_in,
                                                           const int* __restrict__ nmatched, double* __restrict__ ap,
                                                           float* __restrict__ prec_ws, int* __restrict__ cum_ws) {
  __shared__ float sh[MT / 64];
  __shared__ double red[MT / 64];
  __shared__ int tot[2];
  __shared__ float cmx;
  const int s = blockIdx.x, v = blockIdx.y, tid = threadIdx.x;
  const int P = npred[s];
  const int Gv = v == 4 ? nmatched[s] : ngt[s];
  const long po = pred_off[s];
  const unsigned char* cat = cat_in + po;
  const unsigned char* aux = aux_in + po;
  float* prec = prec_ws + (long)v * ptot + po;
  int* cum = cum_ws + (long)v * ptot + po;
  // B: rank among the kept predictions, running TP count, precision
  int carry_k = 0, carry_t = 0;
  for (int c0 = 0; c0 < P; c0 += MT) {
    const int p = c0 + tid;
    bool keep = false, tp = false;
    if (p < P) variant_masks(v, cat[p], aux[p], keep, tp);
    const int rank = (int)block_scan<false>(keep ? 1.f : 0.f, sh) + carry_k;  // counts <= 2^24: exact in f32
    const int inc = (int)block_scan<false>(tp ? 1.f : 0.f, sh) + carry_t;
    if (p < P) {
      cum[p] = inc;
      prec[p] = keep ? (float)inc / ((float)rank + 1e-9f) : 0.f;  // a dropped prediction: neutral in the max
    }
    if (tid == MT - 1) {
      tot[0] = rank;
      tot[1] = inc;
    }
    __syncthreads();
    carry_k = tot[0];
    carry_t = tot[1];
    __syncthreads();
  }
  if (carry_k == 0 || Gv == 0) {  // eval_vit.py:209-214 on the variant's own counts (block-uniform)
    if (tid == 0) ap[(long)s * NVAR + v] = (carry_k == 0 && Gv == 0) ? 1.0 : 0.0;
    return;
  }
  // C: suffix max of precision, VOC sum over the TP positions (f64)
  const float ng = (float)Gv + 1e-9f;
  float smax = 0.f;
  double acc = 0.0;
  const int nch = (P + MT - 1) / MT;
  for (int ch = nch - 1; ch >= 0; --ch) {
    const int p = ch * MT + (MT - 1 - tid);  // reverse order inside the chunk
    const float pv = p < P ? prec[p] : 0.f;
    const float m = fmaxf(block_scan<true>(pv, sh), smax);
    if (p < P) {
      bool keep, tp;
      variant_masks(v, cat[p], aux[p], keep, tp);
      if (tp) {
        const int c = cum[p];
        const double r1 = (double)((float)c / ng), r0 = (double)((float)(c - 1) / ng);
        acc += (r1 - r0) * (double)m;
      }
    }
    if (tid == MT - 1) cmx = m;
    __syncthreads();
    smax = cmx;
    __syncthreads();
  }
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double a = 0.0;
    for (int i = 0; i < MT / 64; ++i) a += red[i];
    ap[(long)s * NVAR + v] = a;
  }
}

// prec f32 + cum i32 per (variant, prediction), matched count per sample, aux byte per prediction
inline long errors_ws_bytes(long n_samples, long total_pred) {
  const long tp = total_pred > 0 ? total_pred : 1, ns = n_samples > 0 ? n_samples : 1;
  return 8 * NVAR * tp + 4 * ns + tp;
}

}  // namespace

extern "C" long ivit_det_errors_workspace(long n_samples, long total_pred) {
  return errors_ws_bytes(n_samples, total_pred);
}

extern "C" int ivit_det_errors(const float* iou, const long* iou_off, const int* npred, const int* ngt,
                               const long* pred_off, const long* gt_off, long n_samples, long total_pred,
                               const float* pred_boxes, const float* gt_boxes, const int* pred_int,
                               const int* gt_int, float thr_fg, float thr_bg, const float* range_edges,
                               int n_edges, unsigned char* category, unsigned char* gt_status, int* best_gt,
                               double* errors, double* tallies, int* confusion, double* ap, void* work,
                               long work_bytes, int max_gt, void* stream) {
  IVIT_CHECK_ARG(max_gt <= MAX_GT, "ivit_det_errors: at most %d GT boxes per sample (got %d)", MAX_GT, max_gt);
  IVIT_CHECK_ARG(n_edges >= 0 && n_edges <= MAX_BINS - 1, "ivit_det_errors: at most %d range bins (%d edges; got %d edges)",
                 MAX_BINS, MAX_BINS - 1, n_edges);
  IVIT_CHECK_ARG(n_edges == 0 || range_edges != nullptr, "ivit_det_errors: range edges missing");
  Edges ed;
  ed.n = n_edges;
  for (int i = 0; i < MAX_BINS - 1; ++i) ed.e[i] = i < n_edges ? range_edges[i] : 0.f;
  for (int i = 1; i < n_edges; ++i)
    IVIT_CHECK_ARG(ed.e[i] > ed.e[i - 1], "ivit_det_errors: range edges must be ascending (edge %d: %g after %g)", i,
                   (double)ed.e[i], (double)ed.e[i - 1]);
  IVIT_CHECK_ARG(thr_bg >= 0.f && thr_bg < thr_fg, "ivit_det_errors: thresholds need 0 <= thr_bg < thr_fg (got %g, %g)",
                 (double)thr_bg, (double)thr_fg);
  IVIT_CHECK_ARG(n_samples < 2147483647L, "ivit_det_errors: grid too large");
  IVIT_CHECK_ARG(work_bytes >= errors_ws_bytes(n_samples, total_pred), "ivit_det_errors: workspace too small");
  if (n_samples <= 0) return 0;
  const long tp = total_pred > 0 ? total_pred : 1;
  float* prec = (float*)work;
  int* cum = (int*)(prec + NVAR * tp);
  int* nmatched = cum + NVAR * tp;
  unsigned char* aux = (unsigned char*)(nmatched + n_samples);
  hipStream_t st = ivit_stream(stream);
  hipLaunchKernelGGL(det_errors_kernel, dim3(n_samples), dim3(MT), 0, st, iou, iou_off, npred, ngt, pred_off, gt_off,
                     pred_boxes, gt_boxes, pred_int, gt_int, thr_fg, thr_bg, ed, category, gt_status, best_gt, errors,
                     tallies, confusion, aux, nmatched);
  IVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(det_errors_ap_kernel, dim3(n_samples, NVAR), dim3(MT), 0, st, npred, ngt, pred_off, tp, category,
                     aux, nmatched, ap, prec, cum);
  IVIT_LAUNCH_CHECK();
  return 0;
}
