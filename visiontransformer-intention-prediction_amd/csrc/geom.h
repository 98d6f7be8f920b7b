// Box geometry device functions shared by the loss and the eval kernels (utils.py).
// Bit-exactness with the reference's f32 tensor arithmetic requires no FMA contraction:
// every file including this header compiles with `#pragma clang fp contract(off)`.
//
// hipcc compiles the header as device code for the library; any C++17 compiler takes it as plain
// host code (tools/geom_host.cpp), so the clip runs under host sanitizers, as geom_ad.h does.
#pragma once
#if defined(__HIPCC__)
#include "ivit_common.h"
#else
#include <math.h>
#define IVIT_DEV inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ivit {

// utils.py:276-292 compute_axis_aligned_iou (cx, cy, w, h): corners by /2, inter via
// clamp(min=0), union = (a1 + a2) - inter, iou = inter / (union + 1e-7).
IVIT_DEV float axis_iou(const float* a, const float* b) {
  const float ax1 = a[0] - a[2] / 2.f, ay1 = a[1] - a[3] / 2.f, ax2 = a[0] + a[2] / 2.f, ay2 = a[1] + a[3] / 2.f;
  const float bx1 = b[0] - b[2] / 2.f, by1 = b[1] - b[3] / 2.f, bx2 = b[0] + b[2] / 2.f, by2 = b[1] + b[3] / 2.f;
  const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f);
  const float ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
  const float inter = iw * ih;
  const float a1 = a[2] * a[3], a2 = b[2] * b[3];
  const float uni = (a1 + a2) - inter;
  return inter / (uni + 1e-7f);
}

// ---- rotated IoU (utils.py:295-392): rectangle corners [-w/2,-l/2],[w/2,-l/2],[w/2,l/2],
// [-w/2,l/2] rotated by yaw about (cx, cy); convex clipping in double (GEOS computes in double).
struct Poly {
  int n;
  double x[12], y[12];
};

IVIT_DEV void rect_poly(const float* b, Poly& p) {
  const double cx = b[0], cy = b[1], hw = (double)b[2] / 2.0, hl = (double)b[3] / 2.0, a = b[4];
  const double c = cos(a), s = sin(a);
  const double lx[4] = {-hw, hw, hw, -hw}, ly[4] = {-hl, -hl, hl, hl};
  p.n = 4;
  for (int i = 0; i < 4; ++i) {
    p.x[i] = lx[i] * c - ly[i] * s + cx;
    p.y[i] = lx[i] * s + ly[i] * c + cy;
  }
}

// Shoelace sum about the first vertex (p.n >= 1): the products are of the size of the polygon, not
// of its distance from the origin. Taken about the origin, a 1 m^2 box at |x|, |y| ~ 1e4 m lost
// 1e-8 m^2 to the cancellation of products near 1e8.
IVIT_DEV double poly_area_signed(const Poly& p) {
  const double x0 = p.x[0], y0 = p.y[0];
  double s = 0.0;
  for (int i = 0; i < p.n; ++i) {
    const int j = (i + 1) % p.n;
    s += (p.x[i] - x0) * (p.y[j] - y0) - (p.y[i] - y0) * (p.x[j] - x0);
  }
  return 0.5 * s;
}

IVIT_DEV void make_ccw(Poly& p) {
  if (poly_area_signed(p) < 0.0) {
    for (int i = 0; i < p.n / 2; ++i) {
      const int j = p.n - 1 - i;
      double t = p.x[i]; p.x[i] = p.x[j]; p.x[j] = t;
      t = p.y[i]; p.y[i] = p.y[j]; p.y[j] = t;
    }
  }
}

// Sutherland-Hodgman: clip P (ccw) by convex Q (ccw); result in P.
IVIT_DEV void clip_poly(Poly& P, const Poly& Q) {
  Poly out;
  for (int e = 0; e < Q.n && P.n > 0; ++e) {
    const double ax = Q.x[e], ay = Q.y[e], bx = Q.x[(e + 1) % Q.n], by = Q.y[(e + 1) % Q.n];
    const double ex = bx - ax, ey = by - ay;
    out.n = 0;
    for (int j = 0; j < P.n; ++j) {
      const int pj = (j + P.n - 1) % P.n;
      const double cxp = P.x[j], cyp = P.y[j], pxp = P.x[pj], pyp = P.y[pj];
      const double sc = ex * (cyp - ay) - ey * (cxp - ax);
      const double sp = ex * (pyp - ay) - ey * (pxp - ax);
      if (sc >= 0.0) {
        if (sp < 0.0 && out.n < 12) {
          const double t = sp / (sp - sc);
          out.x[out.n] = pxp + t * (cxp - pxp);
          out.y[out.n] = pyp + t * (cyp - pyp);
          ++out.n;
        }
        if (out.n < 12) { out.x[out.n] = cxp; out.y[out.n] = cyp; ++out.n; }
      } else if (sp >= 0.0 && out.n < 12) {
        const double t = sp / (sp - sc);
        out.x[out.n] = pxp + t * (cxp - pxp);
        out.y[out.n] = pyp + t * (cyp - pyp);
        ++out.n;
      }
    }
    P = out;
  }
}

// A box prepared once for many pair tests: rect_poly's corners put in ccw order, and the area taken
// BEFORE the reordering (the shoelace sum of the reversed polygon rounds differently).
IVIT_DEV double rect_prepare(const float* b, Poly& p) {
  rect_poly(b, p);
  const double A = fabs(poly_area_signed(p));
  make_ccw(p);
  return A;
}

// IoU of two prepared boxes (rect_prepare): pa is clipped by pb, so the argument order is part of
// the result's last bits. Area / intersection / union guards return 0.
IVIT_DEV float rotated_iou(const Poly& pa, double A1, const Poly& pb, double A2) {
  if (A1 < 1e-6 || A2 < 1e-6) return 0.f;
  Poly pc = pa;
  clip_poly(pc, pb);
  const double inter = pc.n >= 3 ? fabs(poly_area_signed(pc)) : 0.0;
  if (!(inter > 1e-7)) return 0.f;
  const double u = A1 + A2 - inter;
  if (!(u > 1e-6)) return 0.f;
  return (float)(inter / u);
}

IVIT_DEV float rotated_iou(const float* a, const float* b) {
  Poly pa, pb;
  const double A1 = rect_prepare(a, pa), A2 = rect_prepare(b, pb);
  return rotated_iou(pa, A1, pb, A2);
}

}  // namespace ivit
