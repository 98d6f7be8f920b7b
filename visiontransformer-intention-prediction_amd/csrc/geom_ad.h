// IoU of two rotated boxes together with its gradient with respect to the first box, in one
// pass: forward-mode differentiation of geom.h's construction (rect_poly's corner order,
// Sutherland-Hodgman clipping of the predicted rectangle by the target's edges, shoelace areas,
// the same area / intersection / union guards). Every scalar that depends on the predicted box
// (x, y, w, l, yaw) is a value plus five tangents; the target polygon stays plain double.
//
// The header has no HIP dependency: hipcc compiles it as device (and host) code for the library,
// any C++17 compiler as plain host code, so the math runs under host sanitizers
// (tools/riou_host.cpp). No FMA contraction, like geom.h, so both builds round alike.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define IVIT_AD_HD __host__ __device__ inline
#else
#define IVIT_AD_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ivit {
namespace ad {

constexpr int NT = 5;    // tangents: d/dx, d/dy, d/dw, d/dl, d/dyaw of the predicted box
constexpr int MAXV = 8;  // a rectangle clipped by four half-planes gains at most one vertex per plane

struct Dual {
  double v;
  double d[NT];
};

IVIT_AD_HD Dual dconst(double v) {
  Dual r;
  r.v = v;
  for (int k = 0; k < NT; ++k) r.d[k] = 0.0;
  return r;
}
IVIT_AD_HD Dual dvar(double v, int k, double seed) {
  Dual r = dconst(v);
  r.d[k] = seed;
  return r;
}
IVIT_AD_HD Dual operator+(const Dual& a, const Dual& b) {
  Dual r;
  r.v = a.v + b.v;
  for (int k = 0; k < NT; ++k) r.d[k] = a.d[k] + b.d[k];
  return r;
}
IVIT_AD_HD Dual operator-(const Dual& a, const Dual& b) {
  Dual r;
  r.v = a.v - b.v;
  for (int k = 0; k < NT; ++k) r.d[k] = a.d[k] - b.d[k];
  return r;
}
IVIT_AD_HD Dual operator-(const Dual& a, double b) {
  Dual r = a;
  r.v = a.v - b;
  return r;
}
IVIT_AD_HD Dual operator+(const Dual& a, double b) {
  Dual r = a;
  r.v = a.v + b;
  return r;
}
IVIT_AD_HD Dual operator*(const Dual& a, const Dual& b) {
  Dual r;
  r.v = a.v * b.v;
  for (int k = 0; k < NT; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k];
  return r;
}
IVIT_AD_HD Dual operator*(double a, const Dual& b) {
  Dual r;
  r.v = a * b.v;
  for (int k = 0; k < NT; ++k) r.d[k] = a * b.d[k];
  return r;
}
IVIT_AD_HD Dual operator/(const Dual& a, const Dual& b) {
  Dual r;
  r.v = a.v / b.v;
  for (int k = 0; k < NT; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) / b.v;
  return r;
}
IVIT_AD_HD Dual dabs(const Dual& a) { return a.v < 0.0 ? -1.0 * a : a; }

IVIT_AD_HD bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }  // false for NaN, +-Inf

struct PolyD {
  int n;
  Dual x[MAXV], y[MAXV];
};

// rect_poly's corners [-w/2,-l/2], [w/2,-l/2], [w/2,l/2], [-w/2,l/2] rotated by yaw about (x, y)
IVIT_AD_HD void rect_poly_ad(const double* b, PolyD& p) {
  const Dual cx = dvar(b[0], 0, 1.0), cy = dvar(b[1], 1, 1.0);
  const Dual hw = dvar(b[2] / 2.0, 2, 0.5), hl = dvar(b[3] / 2.0, 3, 0.5);
  const double cv = cos(b[4]), sv = sin(b[4]);
  const Dual c = dvar(cv, 4, -sv), s = dvar(sv, 4, cv);
  const double sx[4] = {-1.0, 1.0, 1.0, -1.0}, sy[4] = {-1.0, -1.0, 1.0, 1.0};
  p.n = 4;
  for (int i = 0; i < 4; ++i) {
    const Dual lx = sx[i] * hw, ly = sy[i] * hl;
    p.x[i] = lx * c - ly * s + cx;
    p.y[i] = lx * s + ly * c + cy;
  }
}

IVIT_AD_HD void rect_poly_plain(const double* b, double* qx, double* qy) {
  const double hw = b[2] / 2.0, hl = b[3] / 2.0;
  const double c = cos(b[4]), s = sin(b[4]);
  const double lx[4] = {-hw, hw, hw, -hw}, ly[4] = {-hl, -hl, hl, hl};
  for (int i = 0; i < 4; ++i) {
    qx[i] = lx[i] * c - ly[i] * s + b[0];
    qy[i] = lx[i] * s + ly[i] * c + b[1];
  }
}

IVIT_AD_HD Dual poly_area_signed_ad(const PolyD& p) {
  Dual s = dconst(0.0);
  for (int i = 0; i < p.n; ++i) {
    const int j = i + 1 == p.n ? 0 : i + 1;
    s = s + (p.x[i] * p.y[j] - p.y[i] * p.x[j]);
  }
  return 0.5 * s;
}

IVIT_AD_HD void reverse_ad(PolyD& p) {
  for (int i = 0; i < p.n / 2; ++i) {
    const int j = p.n - 1 - i;
    Dual t = p.x[i]; p.x[i] = p.x[j]; p.x[j] = t;
    t = p.y[i]; p.y[i] = p.y[j]; p.y[j] = t;
  }
}

// Sutherland-Hodgman: clip P (ccw) by the convex quadrilateral Q (ccw, plain double); result in P.
IVIT_AD_HD void clip_poly_ad(PolyD& P, const double* qx, const double* qy) {
  PolyD out;
  for (int e = 0; e < 4 && P.n > 0; ++e) {
    const int e1 = e == 3 ? 0 : e + 1;
    const double ax = qx[e], ay = qy[e];
    const double ex = qx[e1] - ax, ey = qy[e1] - ay;
    out.n = 0;
    for (int j = 0; j < P.n; ++j) {
      const int pj = j == 0 ? P.n - 1 : j - 1;
      const Dual cxp = P.x[j], cyp = P.y[j], pxp = P.x[pj], pyp = P.y[pj];
      const Dual sc = ex * (cyp - ay) - ey * (cxp - ax);
      const Dual sp = ex * (pyp - ay) - ey * (pxp - ax);
      if (sc.v >= 0.0) {
        if (sp.v < 0.0 && out.n < MAXV) {
          const Dual t = sp / (sp - sc);
          out.x[out.n] = pxp + t * (cxp - pxp);
          out.y[out.n] = pyp + t * (cyp - pyp);
          ++out.n;
        }
        if (out.n < MAXV) { out.x[out.n] = cxp; out.y[out.n] = cyp; ++out.n; }
      } else if (sp.v >= 0.0 && out.n < MAXV) {
        const Dual t = sp / (sp - sc);
        out.x[out.n] = pxp + t * (cxp - pxp);
        out.y[out.n] = pyp + t * (cyp - pyp);
        ++out.n;
      }
    }
    P.n = out.n;
    for (int j = 0; j < out.n; ++j) { P.x[j] = out.x[j]; P.y[j] = out.y[j]; }
  }
}

// IoU(p, g) and dIoU/dp (x, y, w, l, yaw) of boxes p (predicted) and g (constant target).
// rotated_iou's guards: either area < 1e-6, intersection <= 1e-7 or union <= 1e-6 give IoU 0 with
// gradient exactly 0. A non-finite coordinate of either box gives NaN for all six numbers (the
// guards' comparisons are false on NaN and would otherwise report "IoU 0").
IVIT_AD_HD void riou_grad(const double* p, const double* g, double* iou, double* grad) {
  bool fin = true;
  for (int k = 0; k < 5; ++k) fin = fin && finite_d(p[k]) && finite_d(g[k]);
  if (!fin) {
    const double qnan = NAN;
    *iou = qnan;
    for (int k = 0; k < NT; ++k) grad[k] = qnan;
    return;
  }
  *iou = 0.0;
  for (int k = 0; k < NT; ++k) grad[k] = 0.0;
  PolyD P;
  rect_poly_ad(p, P);
  const Dual A1s = poly_area_signed_ad(P);
  const Dual A1 = dabs(A1s);
  double qx[4], qy[4];
  rect_poly_plain(g, qx, qy);
  double A2s = 0.0;
  for (int i = 0; i < 4; ++i) {
    const int j = i == 3 ? 0 : i + 1;
    A2s += qx[i] * qy[j] - qy[i] * qx[j];
  }
  A2s = 0.5 * A2s;
  const double A2 = fabs(A2s);
  if (A1.v < 1e-6 || A2 < 1e-6) return;
  if (A1s.v < 0.0) reverse_ad(P);
  if (A2s < 0.0) {
    double t = qx[0]; qx[0] = qx[3]; qx[3] = t;
    t = qx[1]; qx[1] = qx[2]; qx[2] = t;
    t = qy[0]; qy[0] = qy[3]; qy[3] = t;
    t = qy[1]; qy[1] = qy[2]; qy[2] = t;
  }
  clip_poly_ad(P, qx, qy);
  if (P.n < 3) return;
  const Dual inter = dabs(poly_area_signed_ad(P));
  if (!(inter.v > 1e-7)) return;
  const Dual u = A1 + A2 - inter;
  if (!(u.v > 1e-6)) return;
  const Dual r = inter / u;
  *iou = r.v;
  for (int k = 0; k < NT; ++k) grad[k] = r.d[k];
}

// decode_one's formulas (geometry.hip) in f64 from f32 raw outputs d[6] and an f32 anchor a[5],
// without the final angle wrap (the IoU does not see it; its derivative is 1), and no clamp.
IVIT_AD_HD void decode_f64(const float* d, const float* a, double* box) {
  box[0] = (double)d[0] * (double)a[2] + (double)a[0];
  box[1] = (double)d[1] * (double)a[3] + (double)a[1];
  box[2] = exp((double)d[2]) * (double)a[2];
  box[3] = exp((double)d[3]) * (double)a[3];
  box[4] = (double)a[4] + atan2((double)d[4], (double)d[5]);
}

// Chain rule from dIoU/d(box) to the six raw outputs.
IVIT_AD_HD void decode_chain(const float* d, const float* a, const double* box, const double* gbox, double* graw) {
  graw[0] = gbox[0] * (double)a[2];
  graw[1] = gbox[1] * (double)a[3];
  graw[2] = gbox[2] * box[2];
  graw[3] = gbox[3] * box[3];
  const double d4 = d[4], d5 = d[5];
  const double r2 = d4 * d4 + d5 * d5;
  graw[4] = r2 == 0.0 ? 0.0 : gbox[4] * (d5 / r2);
  graw[5] = r2 == 0.0 ? 0.0 : gbox[4] * (-d4 / r2);
}

}  // namespace ad
}  // namespace ivit
