// The elementwise losses of generalized CPD: l(x, m) and dl/dm(x, m) of the
// table in splatt_amd/gcp.py, shared by gcp.hip (stored entries, root-sorted
// stream) and sgcp.hip (sampled entries and cells). Anonymous namespace, as
// in device_common.hpp: each kernel file gets its own internal copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr double GCP_EPS = 1e-10;   // splatt_amd/gcp.py: EPS
constexpr double GCP_PI = 3.14159265358979323846;

enum GcpLoss : int {
  GAUSSIAN = 0, HUBER, POISSON, POISSON_LOG, BERNOULLI_ODDS, BERNOULLI_LOGIT,
  GAMMA, RAYLEIGH, NLOSS
};

// dl/dm(x, m). `loss` is wave-uniform.
__device__ __forceinline__ double
loss_deriv(int loss, double prm, double x, double m) {
  switch (loss) {
    case GAUSSIAN:
      return 2.0 * (m - x);
    case HUBER: {
      const double r = x - m;
      return fabs(r) <= prm ? -2.0 * r : (r > 0.0 ? -2.0 * prm : 2.0 * prm);
    }
    case POISSON:
      return 1.0 - x / (m + GCP_EPS);
    case POISSON_LOG:
      return exp(m) - x;
    case BERNOULLI_ODDS:
      return 1.0 / (m + 1.0) - x / (m + GCP_EPS);
    case BERNOULLI_LOGIT: {
      const double ex = exp(-fabs(m));
      // sigmoid without overflow: 1/(1+e^-m) for m >= 0, e^m/(1+e^m) below
      return (m >= 0.0 ? 1.0 : ex) / (1.0 + ex) - x;
    }
    case GAMMA: {
      const double t = m + GCP_EPS;
      return -x / (t * t) + 1.0 / t;
    }
    default: {  // RAYLEIGH
      const double t = m + GCP_EPS;
      return 2.0 / t - (GCP_PI / 2.0) * (x * x) / (t * t * t);
    }
  }
}

// l(x, m). `loss` is wave-uniform.
__device__ __forceinline__ double
loss_value(int loss, double prm, double x, double m) {
  switch (loss) {
    case GAUSSIAN: {
      const double d = m - x;
      return d * d;
    }
    case HUBER: {
      const double ar = fabs(x - m);
      return ar <= prm ? ar * ar : 2.0 * prm * ar - prm * prm;
    }
    case POISSON:
      return m - x * log(m + GCP_EPS);
    case POISSON_LOG:
      return exp(m) - x * m;
    case BERNOULLI_ODDS:
      return log(m + 1.0) - x * log(m + GCP_EPS);
    case BERNOULLI_LOGIT:
      return fmax(m, 0.0) + log1p(exp(-fabs(m))) - x * m;
    case GAMMA: {
      const double t = m + GCP_EPS;
      return x / t + log(t);
    }
    default: {  // RAYLEIGH
      const double t = m + GCP_EPS, q = x / t;
      return 2.0 * log(t) + (GCP_PI / 4.0) * (q * q);
    }
  }
}

}  // namespace
