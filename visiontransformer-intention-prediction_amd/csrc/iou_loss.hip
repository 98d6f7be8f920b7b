// Rotated-IoU box regression: the element-wise op (ivit_riou_pairs_*) and the opt-in term of
// DetectionIntentionLoss (ivit_det_iou_loss_*), both on geom_ad.h's one-pass IoU + gradient.
//
// The loss term runs right after ivit_det_loss_fwd on the same stream. For every anchor that
// assign_loss_kernel marked positive (cls target 1 in its `tgt` words) one lane
//   1. re-runs the first-index argmax over the sample's GT boxes with the assignment's own IoU,
//   2. decodes the six raw outputs in f64 (decode_one's formulas, no angle wrap),
//   3. takes IoU_rot(decoded, matched GT) and its gradient, chains it to the raw outputs and stores
//      those six numbers at the anchor's own slot (no compaction: no order reaches an output bit),
//   4. adds (1 - IoU, IoU) to its block's f64 partial sums (fixed-order LDS tree, no atomics).
// A one-block final sums the partials in a fixed order and folds the term into the stats vector.
#include "geom.h"
#include "geom_ad.h"

#pragma clang fp contract(off)

using namespace ivit;

namespace {

// the det-loss stats slots this file reads or writes (loss.hip), plus its own
enum { ST_NPOS = 3, ST_LOSS = 5, ST_CLS = 6, ST_BOXL = 7, ST_INT = 8, ST_FINITE = 9, ST_CDEN = 10,
       ST_IOU_SUM = 12, ST_POSIOU_SUM = 13, ST_IOUL = 14, ST_POSIOU = 15 };
constexpr int LB = 256;

IVIT_DEV float iou_of(const float* a, const float* g, int rot) { return rot ? rotated_iou(a, g) : axis_iou(a, g); }

__global__ __launch_bounds__(LB) void riou_pairs_fwd_kernel(const float* __restrict__ boxes,
                                                            const float* __restrict__ targets, long n,
                                                            float* __restrict__ iou, float* __restrict__ jac) {
  const long i = (long)blockIdx.x * LB + threadIdx.x;
  if (i >= n) return;
  double p[5], g[5], v, gr[5];
  for (int k = 0; k < 5; ++k) { p[k] = boxes[i * 5 + k]; g[k] = targets[i * 5 + k]; }
  ad::riou_grad(p, g, &v, gr);
  iou[i] = (float)v;
  for (int k = 0; k < 5; ++k) jac[i * 5 + k] = (float)gr[k];
}

__global__ __launch_bounds__(LB) void riou_pairs_bwd_kernel(const float* __restrict__ grad_iou,
                                                            const float* __restrict__ jac, long total,
                                                            float* __restrict__ dboxes) {
  const long i = (long)blockIdx.x * LB + threadIdx.x;  // over n * 5
  if (i >= total) return;
  dboxes[i] = grad_iou[i / 5] * jac[i];
}

struct IouWs {
  float* graw;    // [B*NA*6] dIoU/d(raw output) of the positives (other slots unwritten)
  double* part;   // [nblk*2] per-block (sum 1 - IoU, sum IoU)
};

IouWs carve(void* work, long B, long NA) {
  IouWs ws;
  ws.graw = (float*)work;
  ws.part = (double*)((char*)work + (B * NA * 24 + 255) / 256 * 256);
  return ws;
}

__global__ __launch_bounds__(LB) void iou_term_kernel(const float* __restrict__ box, const float* __restrict__ anchors,
                                                      long total, long NA, const float* __restrict__ gt,
                                                      const int* __restrict__ ngt, int G, int rot,
                                                      const int* __restrict__ tgt, IouWs ws) {
  const long i = (long)blockIdx.x * LB + threadIdx.x;  // b * NA + a
  double one_minus = 0.0, iouv = 0.0;
  if (i < total && (tgt[i] & 3) == 2) {
    const int b = (int)(i / NA);
    const long a = i - (long)b * NA;
    const float* an = anchors + a * 5;
    int ng = ngt[b];
    ng = ng < G ? ng : G;
    if (ng > 0) {
      float mx = -1.f;
      int arg = 0;
      for (int g = 0; g < ng; ++g) {
        const float v = iou_of(an, gt + ((long)b * G + g) * 5, rot);
        if (v > mx) { mx = v; arg = g; }
      }
      const float* gb = gt + ((long)b * G + arg) * 5;
      const float* d = box + i * 6;
      double p[5], q[5], gr[5], graw[6];
      ad::decode_f64(d, an, p);
      for (int k = 0; k < 5; ++k) q[k] = gb[k];
      ad::riou_grad(p, q, &iouv, gr);
      ad::decode_chain(d, an, p, gr, graw);
      for (int k = 0; k < 6; ++k) ws.graw[i * 6 + k] = (float)graw[k];
      one_minus = 1.0 - iouv;
    } else {
      for (int k = 0; k < 6; ++k) ws.graw[i * 6 + k] = 0.f;  // a positive without GT: not produced by the assignment
    }
  }
  __shared__ double red[2][LB];
  red[0][threadIdx.x] = one_minus;
  red[1][threadIdx.x] = iouv;
  __syncthreads();
  for (int o = LB / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) ws.part[(long)blockIdx.x * 2 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void iou_final_kernel(const double* __restrict__ part, int nblk, float wb, float lam,
                                                        float* stats) {
  __shared__ double red[2][256];
  double s0 = 0.0, s1 = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) { s0 += part[(long)k * 2]; s1 += part[(long)k * 2 + 1]; }
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x) return;
  stats[ST_IOU_SUM] = (float)red[0][0];
  stats[ST_POSIOU_SUM] = (float)red[1][0];
  stats[ST_IOUL] = 0.f;
  stats[ST_POSIOU] = 0.f;
  if (stats[ST_FINITE] == 0.f) return;  // the guard already fired: it stays fired, terms stay 0
  const float npos = stats[ST_NPOS], cden = stats[ST_CDEN];
  const float il = npos > 0.f ? (float)((double)lam * red[0][0] / (double)cden) : 0.f;
  const float pi = npos > 0.f ? (float)(red[1][0] / (double)cden) : 0.f;
  const float bl = stats[ST_BOXL] + il;
  const float tot = stats[ST_LOSS] + wb * il;
  const bool fin = isfinite(tot);
  stats[ST_LOSS] = fin ? tot : 0.f;
  stats[ST_BOXL] = fin ? bl : 0.f;
  stats[ST_IOUL] = fin ? il : 0.f;
  stats[ST_POSIOU] = fin ? pi : 0.f;
  if (!fin) {
    stats[ST_CLS] = 0.f;
    stats[ST_INT] = 0.f;
    stats[ST_FINITE] = 0.f;
  }
}

__global__ __launch_bounds__(LB) void iou_term_bwd_kernel(long total, float wb, float lam,
                                                          const float* __restrict__ stats, const float* grad_loss,
                                                          const int* __restrict__ tgt, const float* __restrict__ graw,
                                                          float* dbox) {
  const long i = (long)blockIdx.x * LB + threadIdx.x;
  if (i >= total) return;
  if (stats[ST_FINITE] == 0.f) return;  // ivit_det_loss_bwd wrote exact zeros: add nothing
  if ((tgt[i] & 3) != 2) return;
  const float go = grad_loss ? grad_loss[0] : 1.f;
  const float sc = go * wb * lam / stats[ST_CDEN];
  for (int k = 0; k < 6; ++k) dbox[i * 6 + k] += sc * -graw[i * 6 + k];
}

}  // namespace

extern "C" int ivit_riou_pairs_fwd(const float* boxes, const float* targets, long n, float* iou, float* jac,
                                   void* stream) {
  IVIT_CHECK_ARG(n >= 0, "ivit_riou_pairs_fwd: n >= 0");
  if (n == 0) return 0;
  IVIT_CHECK_ARG(boxes && targets && iou && jac, "ivit_riou_pairs_fwd: null pointer with n > 0");
  IVIT_CHECK_ARG(n <= (1L << 31) * 50, "ivit_riou_pairs_fwd: n too large for one launch");
  hipLaunchKernelGGL(riou_pairs_fwd_kernel, dim3(ivit_cdiv(n, LB)), dim3(LB), 0, ivit_stream(stream), boxes, targets,
                     n, iou, jac);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_riou_pairs_bwd(const float* grad_iou, const float* jac, long n, float* dboxes, void* stream) {
  IVIT_CHECK_ARG(n >= 0, "ivit_riou_pairs_bwd: n >= 0");
  if (n == 0) return 0;
  IVIT_CHECK_ARG(grad_iou && jac && dboxes, "ivit_riou_pairs_bwd: null pointer with n > 0");
  IVIT_CHECK_ARG(n <= (1L << 31) * 50, "ivit_riou_pairs_bwd: n too large for one launch");
  hipLaunchKernelGGL(riou_pairs_bwd_kernel, dim3(ivit_cdiv(n * 5, LB)), dim3(LB), 0, ivit_stream(stream), grad_iou, jac,
                     n * 5, dboxes);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" long ivit_det_iou_loss_workspace(long B, long NA) {
  if (B <= 0 || NA <= 0) return 0;
  return (B * NA * 24 + 255) / 256 * 256 + ((long)ivit_cdiv(B * NA, LB) * 16 + 255) / 256 * 256;
}

extern "C" int ivit_det_iou_loss_fwd(const float* box, const float* anchors, long B, long NA, const float* gt,
                                     const int* ngt, long Gmax, int use_rotated, float w_box, float iou_weight,
                                     const void* det_work, long det_work_bytes, float* stats, void* work,
                                     long work_bytes, void* stream) {
  IVIT_CHECK_ARG(B >= 0 && NA >= 0 && Gmax >= 0, "ivit_det_iou_loss_fwd: negative size");
  if (B == 0 || NA == 0) return 0;
  IVIT_CHECK_ARG(B * NA <= (1L << 31) - 1, "ivit_det_iou_loss_fwd: B * NA < 2^31");
  IVIT_CHECK_ARG(box && anchors && ngt && det_work && stats && work && (gt || Gmax == 0),
                 "ivit_det_iou_loss_fwd: null pointer");
  IVIT_CHECK_ARG(det_work_bytes >= B * NA * 4, "ivit_det_iou_loss_fwd: det-loss workspace too small");
  IVIT_CHECK_ARG(work_bytes >= ivit_det_iou_loss_workspace(B, NA), "ivit_det_iou_loss_fwd: workspace too small");
  hipStream_t st = ivit_stream(stream);
  IouWs ws = carve(work, B, NA);
  const long total = B * NA;
  const int nblk = ivit_cdiv(total, LB);
  hipLaunchKernelGGL(iou_term_kernel, dim3(nblk), dim3(LB), 0, st, box, anchors, total, NA, gt, ngt, (int)Gmax,
                     use_rotated, (const int*)det_work, ws);
  hipLaunchKernelGGL(iou_final_kernel, dim3(1), dim3(256), 0, st, (const double*)ws.part, nblk, w_box, iou_weight,
                     stats);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_det_iou_loss_bwd(long B, long NA, float w_box, float iou_weight, const float* stats,
                                     const float* grad_loss, const void* det_work, long det_work_bytes,
                                     const void* work, long work_bytes, float* dbox, void* stream) {
  IVIT_CHECK_ARG(B >= 0 && NA >= 0, "ivit_det_iou_loss_bwd: negative size");
  if (B == 0 || NA == 0) return 0;
  IVIT_CHECK_ARG(B * NA <= (1L << 31) - 1, "ivit_det_iou_loss_bwd: B * NA < 2^31");
  IVIT_CHECK_ARG(stats && det_work && work && dbox, "ivit_det_iou_loss_bwd: null pointer");
  IVIT_CHECK_ARG(det_work_bytes >= B * NA * 4, "ivit_det_iou_loss_bwd: det-loss workspace too small");
  IVIT_CHECK_ARG(work_bytes >= ivit_det_iou_loss_workspace(B, NA), "ivit_det_iou_loss_bwd: workspace too small");
  const long total = B * NA;
  hipLaunchKernelGGL(iou_term_bwd_kernel, dim3(ivit_cdiv(total, LB)), dim3(LB), 0, ivit_stream(stream), total, w_box,
                     iou_weight, stats, grad_loss, (const int*)det_work, (const float*)work, dbox);
  IVIT_LAUNCH_CHECK();
  return 0;
}
