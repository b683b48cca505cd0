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
    if (arg < 100.0) {
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
    const double r1 = rate > 0.0 ? sig / safe : 1.0;                // rate' / rate
    const double r2 = rate > 0.0 ? (dsig * safe - sig * sig) / (safe * safe) : 0.0;
    g = y * r1 - sig;
    h = y * r2 - dsig;
  }
}
