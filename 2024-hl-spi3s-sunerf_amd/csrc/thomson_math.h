// The Thomson-scattering intensities of one electron (Howard & Tappin 2009, eqs. 23, 24, 29): the one text behind the samples of
// the white-light integral (thomson.hip) and the polarisation ratio that polarimetry.hip inverts.  With R the solar radius, r > R
// the electron's distance from the Sun's centre, u the limb-darkening coefficient and p2 the squared impact parameter of the line
// of sight (sin^2(chi) = p2 / r^2):
//
//   s = sin(Omega) = R / r,  c = cos(Omega),  L = ln((1 + s) / c) = atanh(s)
//   A = c s^2                      B = -(1/8) (1 - 3 s^2 - (c^2 / s)(1 + 3 s^2) L)
//   C = 4/3 - c - c^3/3            D = (1/8) (5 + s^2 - (c^2 / s)(5 - s^2) L)
//   I_T = (1-u) C + u D,   I_P = sin^2(chi) ((1-u) A + u B),   I_tot = 2 I_T - I_P
//
// Numerics: A..D are differences that cancel to O(s^2) far from the Sun (C ~ s^2, B ~ D ~ 2/3 s^2); all of it is fp64, C in the
// cancellation-free form (1 - c)(4 + c + c^2) / 3 with 1 - c = s^2 / (1 + c), L as log1p, c^2 as (r^2 - R^2) / r^2: the residual
// relative error is ~1e-16 / s^2.  Every operation is rounded on its own (-ffp-contract=off), in the order written: the callers'
// results are functions of this text alone.
#pragma once

struct ThomsonIntensity {
  double i_tot, i_p;         // signed, as the formulas give them
};

// r2 = r^2 as the caller formed it, r = sqrt(r2) > R
__device__ __forceinline__ ThomsonIntensity thomson_intensity(double r2, double r, double R, double u, double p2) {
  const double s = R / r, s2 = s * s;
  // cos^2 from the squares: r^2 - R^2 is exact next to the limb, where 1 - s^2 keeps only the rounding of r (1e-3 of c one
  // fp32 step of z outside a limb at R = 1 / 0.7, and with it of I_P = c s^2 sin^2(chi) at u = 0).  r > R gives r^2 > R^2.
  const double c2 = (r2 - R * R) / r2, c = sqrt(c2);
  const double L = 0.5 * log1p(2.0 * s / (1.0 - s));   // ln((1 + s) / c)
  const double k = c2 * r / R * L;                      // (c^2 / s) L
  const double A = c * s2;
  const double B = -0.125 * ((1.0 - 3.0 * s2) - k * (1.0 + 3.0 * s2));
  const double Cc = s2 / (1.0 + c) * (4.0 + c + c2) / 3.0;   // 4/3 - c - c^3/3
  const double D = 0.125 * ((5.0 + s2) - k * (5.0 - s2));
  const double sin2chi = p2 / r2;
  const double it = (1.0 - u) * Cc + u * D;
  ThomsonIntensity o;
  o.i_p = sin2chi * ((1.0 - u) * A + u * B);
  o.i_tot = 2.0 * it - o.i_p;
  return o;
}
