// lik_point.h -- the per-point log-likelihood of the logistic / Poisson regression models in its linear predictor, with its
// first two derivatives: ONE text for the Laplace sampler (csrc/laplace.hip) and the log joint / HMC kernels (csrc/hmc.hip).
#pragma once
#include <hip/hip_runtime.h>

enum { LAP_LOGISTIC = 0, LAP_POISSON = 1 };

// d/ds and d^2/ds^2 of the log-likelihood in the linear predictor s, and the log-likelihood itself (constants in theta dropped)
static __device__ __forceinline__ void lap_point(int family, double s, double y, double& ll, double& g, double& h) {
  if (family == LAP_LOGISTIC) {
    // log p = -log(1 + exp(-s)), linear tail beyond -s >= 100 (model_lr.py:29-31)
    const double arg = -s;
    if (!(arg >= 100.0)) {                                          // (a NaN predictor goes through exp: NaN in ll, g and h)
      const double e = exp(arg);
      ll = -log1p(e);
      g = e / (1.0 + e);
      h = -e / ((1.0 + e) * (1.0 + e));
    } else { ll = -arg; g = 1.0; h = 0.0; }
  } else {
    // rate = log(1 + e^s); log p = y log rate - rate (- log y!); log rate = s where rate = e^s to every bit (model_poiss.py:25-38)
    const double e = exp(-fabs(s));
    const double rate = fmax(s, 0.0) + log1p(e);
    const double lr = s > -100.0 ? log(rate > 0.0 ? rate : 1.0) : s;
    ll = y * lr - rate;
    const double sig = (s >= 0.0 ? 1.0 : e) / (1.0 + e);           // rate'
    const double dsig = e / ((1.0 + e) * (1.0 + e));                // rate''
    const double safe = rate > 0.0 ? rate : 1.0;
    // Below s = -300 the rate is e^s (1 - e^s / 2 + ..): rate' / rate = 1 and (rate'' rate - rate'^2) / rate^2 = -e^s / 2 to every
    // bit, and neither quotient may be formed there.  e^s is subnormal below s = -708 (exp, log1p and the division then agree
    // to one part in 2^37 at best: y times that in g), rate^2 leaves the normal range at s = -354 and is 0 from -372.5 on (0 / 0).
    const bool body = rate > 0.0 && !(s < -300.0);
    const double r1 = body ? sig / safe : 1.0;                      // rate' / rate
    const double r2 = body ? (dsig * safe - sig * sig) / (safe * safe) : (rate > 0.0 ? -0.5 * e : 0.0);
    g = y * r1 - sig;
    h = y * r2 - dsig;
  }
}
