// iem_qf_device.h — the kernels of the iem_qf object (include/iem.h): the QUALITY-FUNCTION oracle of the adaptive barrier parameter on
// the blocks of an iem_amu and its iem_mu — the residual norms the quality function scales (qf_begin), the fraction-to-the-boundary
// step lengths of the direction at a candidate sigma (qf_alpha), the quality function there together with ONE step of the section
// search over sigma (qf_value), and the rule (qf_update): amu_update of iem_amu_device.h word for word with the section's result as
// the free-mode oracle.  A code object of its own (no other source key knows of it), compiled with -ffp-contract=off behind the
// helpers of iem_device.h (everything in front of its own kernels, with IEM_TILE = 256): every line below is the order of operations
// of the contract in include/iem.h, each operation rounded once.
//
// NO FLOAT ATOMIC, no inline assembly, no scratch, no cooperative launch and no grid-wide wait in this file: every dependence between
// workgroups is a launch boundary.  The only atomic is the integer atomicMin on the bit pattern of a non-negative double, at most
// ONE per workgroup and slot (the scheme of bar_extremes in iem_barrier_device.h: shuffles, LDS, a relaxed look at the slot).  The
// sums go through iem_shared_park / iem_shared_last / iem_shared_totals of iem_device.h as they stand: a lane adds its entries in
// index order, every workgroup parks its values, the workgroup that arrives last totals each column in a fixed order and — one
// thread — moves the section's state machine.
//
// qf_begin, qf_alpha, qf_value: the grid of the barrier object — one thread takes the entries i, i + stride, ... of [0, nvar + ncon):
// i < nvar is variable i, otherwise row j = i − nvar; flags as in mu_error (fx / fc bit 0 = lower bound present, bit 1 = upper, fc
// bit 2 = equality row).  qf_update, qf_reset: ONE workgroup of 64 threads, one thread decides.

#define QF_IDLE 0ll
#define QF_SECTION 1ll
#define QF_DONE 2ll
#define QF_UNUSABLE 3ll
#define QF_ONE_BITS 0x3ff0000000000000ull   // 1.0
#define QF_INF_BITS 0x7ff0000000000000ll
#define QF_GOLDEN 0.6180339887498949
#define QF_MU_ITERATING 0ll
#define QF_MU_CONVERGED 1ll
#define QF_MU_UNUSABLE 2ll
#define QF_FREE 0ll
#define QF_FIXED 1ll
#define QF_MAX_DECREASES 64
#define QF_REFS 4

// the iem_mu block, the iem_amu block (the words qf_update writes as amu_update does) and the object's own block: words of 8 bytes
enum { QMW_MU, QMW_TAU, QMW_ZETA, QMW_E0, QMW_EMU, QMW_ED, QMW_EP, QMW_EC0, QMW_STATUS, QMW_FLAGS, QMW_DECREASES, QMW_UPDATES };
enum { QAW_MODE, QAW_MU_MAX, QAW_NREFS, QAW_REF0, QAW_MU_ORACLE = 7, QAW_SIGMA, QAW_AVG, QAW_M_AFF, QAW_TO_FIXED, QAW_TO_FREE };
enum { QW_STATUS, QW_PHASE, QW_STEPS, QW_EVALS, QW_SIGMA, QW_ALPHA_P, QW_ALPHA_D, QW_D2, QW_P2, QW_AVG, QW_LO, QW_HI, QW_A, QW_B, QW_C, QW_D,
       QW_QC, QW_QD, QW_BEST, QW_QBEST, QW_Q0, QW_Q, QW_C2, QW_NAN, QW_LAST_AP, QW_LAST_AD, QW_SIGMA0, QW_WORDS = 32 };
// the phase: which evaluation the next alpha / value pair is
enum { QP_FIRST, QP_SECOND, QP_LEFT, QP_RIGHT, QP_NEW_LEFT, QP_NEW_RIGHT };

struct QfArgs {
  const double *xl, *xu, *rl, *ru, *ceq;          // the barrier object's relaxed bounds and the equality rows' right-hand side
  const unsigned char *fx, *fc;
  const double *x, *s, *y, *zL, *zU, *vL, *vU;    // the state
  const double *r, *c;                            // qf_begin: sigma grad f + J'y (nvar), c(x) (ncon)
  const double *sol0, *ds0, *dzL0, *dzU0, *dvL0, *dvU0;      // d0: the direction at mu = 0 (sol = [dx; dy])
  const double *sol1, *ds1, *dzL1, *dzU1, *dvL1, *dvU1;      // d1: the direction at mu = mu_ref
  const double *w;                                // the twelve words of mu_error
  double *mblk;                                   // the iem_mu block
  double *ablk;                                   // the iem_amu block
  double *qblk;                                   // the object's own block
  double *sctl;                                   // qf_update: the control block of a search whose filter a change of mu empties, or null
  double *red;                                    // 2 n_wg parked values, then the ticket words (the object's own)
  const long long *tab;                           // offs[2] | first[2] | count[2] of iem_shared_totals
  double kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max;      // of the iem_mu object
  double mu_min, mu_max_fact, init_factor, red_fact;              // of the iem_amu object
  double mu_ref, sigma_min, sigma_max, sigma_tol;                 // the object's own
  long long max_steps, refs_max, force_fixed;
  long long n_d, n_p;                             // nvar + inequality rows, ncon
  long long ncon, nz;
  long long nvar, n, n_wg;
};

// np.maximum / np.minimum: a NaN in either operand gives a NaN (amu_max / amu_min of iem_amu_device.h)
__device__ __forceinline__ double qf_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double qf_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ long long qf_word(const double *blk, int w) { return __double_as_longlong(blk[w]); }
__device__ __forceinline__ void qf_set_word(double *blk, int w, long long v) { blk[w] = __longlong_as_double(v); }
// a step-length candidate: its bit pattern, or 0 when it is not > 0 (bar_cand of iem_barrier_device.h)
__device__ __forceinline__ unsigned long long qf_cand(double a) { return a > 0.0 ? (unsigned long long)__double_as_longlong(a) : 0ull; }
__device__ __forceinline__ unsigned long long qf_umin(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// THE direction at mu = sigma·avg from the two columns: t = (sigma·avg)/mu_ref once per thread, then per component
//     e = d1 − d0;  d = d0 + t·e
// — the one place where both grid kernels form it
__device__ __forceinline__ double qf_t(const double *qblk, double mu_ref) {
  double t = qblk[QW_SIGMA] * qblk[QW_AVG];
  t = t / mu_ref;
  return t;
}
__device__ __forceinline__ double qf_dir(double d0, double d1, double t) {
  const double e = d1 - d0;
  const double u = t * e;
  return d0 + u;
}

// The two minima of the workgroup into their slots: bar_extremes<2, true> of iem_barrier_device.h
__device__ __forceinline__ void qf_minima(unsigned long long (&v)[2], unsigned long long *slots, unsigned long long *lds) {
  constexpr int NW = IEM_TILE / IEM_WAVE;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    for (int o = 32; o > 0; o >>= 1) v[s] = qf_umin(v[s], __shfl_xor(v[s], o, 64));
    if (iem_lane() == 0) lds[iem_wave() * 2 + s] = v[s];
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int s = (int)threadIdx.x;
    unsigned long long b = lds[s];
    for (int w = 1; w < NW; ++w) b = qf_umin(b, lds[w * 2 + s]);
    const unsigned long long cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b < cur) atomicMin(slots + s, b);
  }
}

// the section starts: the bracket of sigma, the first trial, the alpha slots seeded (one thread)
__device__ __forceinline__ void qf_open(const QfArgs &A, double d2, double p2) {
  double *q = A.qblk;
  for (int w = 0; w < QW_WORDS; ++w) q[w] = 0.0;
  q[QW_D2] = d2;
  q[QW_P2] = p2;
  if (A.nz == 0) { qf_set_word(q, QW_STATUS, QF_DONE); return; }
  const double avg = A.w[9] / (double)A.nz;
  double mu_hi = A.ablk[QAW_MU_MAX];
  if (__double_as_longlong(mu_hi) == 0ll) mu_hi = A.mu_max_fact * avg;
  const double lo = qf_max(A.sigma_min, A.mu_min / avg);
  const double hi = qf_max(lo, qf_min(A.sigma_max, mu_hi / avg));
  const double first = qf_min(qf_max(1.0, lo), hi);
  q[QW_AVG] = avg;
  q[QW_LO] = lo;
  q[QW_HI] = hi;
  q[QW_SIGMA] = first;
  q[QW_SIGMA0] = first;
  qf_set_word(q, QW_ALPHA_P, (long long)QF_ONE_BITS);
  qf_set_word(q, QW_ALPHA_D, (long long)QF_ONE_BITS);
  qf_set_word(q, QW_PHASE, QP_FIRST);
  qf_set_word(q, QW_STATUS, QF_SECTION);
}

extern "C" __global__ __launch_bounds__(256) void qf_begin(const QfArgs A) {
  __shared__ double lds[16];      // 2 (NW + 1) + 1 doubles at least: the parked columns, the totals, the flag
  const long long stride = (long long)gridDim.x * 256;
  double v[2] = {0.0, 0.0};       // D2, P2: the residual expressions of barrier_error, squared
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      double t = A.r[i];
      if (f & 1) t = t - A.zL[i];
      if (f & 2) t = t + A.zU[i];
      v[0] += t * t;
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      double inf;
      if (f & 4) {
        inf = A.c[j] - A.ceq[j];
      } else {
        inf = A.c[j] - A.s[j];
        double t = -A.y[j];
        if (f & 1) t = t - A.vL[j];
        if (f & 2) t = t + A.vU[j];
        v[0] += t * t;
      }
      v[1] += inf * inf;
    }
  }
  iem_shared_park<2>(v, A.red, A.tab, (long long)blockIdx.x, lds);
  if (!iem_shared_last(A.red + 2 * A.n_wg, (long long)blockIdx.x, A.n_wg, lds + 15)) return;
  iem_shared_totals(2, A.red, A.tab, A.tab + 2, A.tab + 4, lds);
  if (threadIdx.x == 0) qf_open(A, lds[0], lds[1]);
}

extern "C" __global__ __launch_bounds__(256) void qf_alpha(const QfArgs A) {
  __shared__ unsigned long long lds[2 * (IEM_TILE / IEM_WAVE)];
  if (qf_word(A.qblk, QW_STATUS) != QF_SECTION) return;      // gated: before the first store
  const long long stride = (long long)gridDim.x * 256;
  const double t = qf_t(A.qblk, A.mu_ref);
  const double tau = A.mblk[QMW_TAU], ntau = -tau;
  unsigned long long ap = QF_ONE_BITS, ad = QF_ONE_BITS;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      const double dx = qf_dir(A.sol0[i], A.sol1[i], t);
      if (dx != dx) ap = 0ull;      // a NaN in the direction: unusable, whatever the bounds
      if (f & 3) {
        const double x = A.x[i];
        if (f & 1) {
          const double d = x - A.xl[i], z = A.zL[i];
          const double dzl = qf_dir(A.dzL0[i], A.dzL1[i], t);
          if (dx < 0.0) ap = qf_umin(ap, qf_cand((ntau * d) / dx));
          if (dzl < 0.0) ad = qf_umin(ad, qf_cand((ntau * z) / dzl));
          if (dzl != dzl) ad = 0ull;
        }
        if (f & 2) {
          const double d = A.xu[i] - x, z = A.zU[i];
          const double dzu = qf_dir(A.dzU0[i], A.dzU1[i], t);
          if (dx > 0.0) ap = qf_umin(ap, qf_cand((tau * d) / dx));
          if (dzu < 0.0) ad = qf_umin(ad, qf_cand((ntau * z) / dzu));
          if (dzu != dzu) ad = 0ull;
        }
      }
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (f & 4) continue;
      const double ds = qf_dir(A.ds0[j], A.ds1[j], t);
      if (ds != ds) ap = 0ull;
      if (f & 3) {
        const double s = A.s[j];
        if (f & 1) {
          const double el = s - A.rl[j], vl = A.vL[j];
          const double dvl = qf_dir(A.dvL0[j], A.dvL1[j], t);
          if (ds < 0.0) ap = qf_umin(ap, qf_cand((ntau * el) / ds));
          if (dvl < 0.0) ad = qf_umin(ad, qf_cand((ntau * vl) / dvl));
          if (dvl != dvl) ad = 0ull;
        }
        if (f & 2) {
          const double eu = A.ru[j] - s, vu = A.vU[j];
          const double dvu = qf_dir(A.dvU0[j], A.dvU1[j], t);
          if (ds > 0.0) ap = qf_umin(ap, qf_cand((tau * eu) / ds));
          if (dvu < 0.0) ad = qf_umin(ad, qf_cand((ntau * vu) / dvu));
          if (dvu != dvu) ad = 0ull;
        }
      }
    }
  }
  unsigned long long a[2] = {ap, ad};      // the slots were seeded with the bits of 1.0 by qf_begin / the last qf_value
  qf_minima(a, reinterpret_cast<unsigned long long *>(A.qblk + QW_ALPHA_P), lds);
}

// one present bound: the square of the product the step would leave, and the count of NaN products (amu_product's order)
__device__ __forceinline__ void qf_product(double (&v)[2], double gap, double t, bool upper, double z, double u) {
  const double g = upper ? gap - t : gap + t;
  const double w = z + u;
  const double p = g * w;
  if (p != p) v[1] += 1.0;
  v[0] += p * p;
}

// ONE step of the section from the value q at the trial sigma (one thread); the next trial and the re-seeded slots
__device__ __forceinline__ void qf_section(const QfArgs &A, double c2, double nan, double ap, double ad) {
  double *b = A.qblk;
  const double sigma = b[QW_SIGMA];
  double q;
  if (__double_as_longlong(ap) == 0ll || __double_as_longlong(ad) == 0ll || nan != 0.0) {
    q = __longlong_as_double(QF_INF_BITS);
  } else {
    const double ud = 1.0 - ad, up = 1.0 - ap;
    const double td = A.n_d ? ((ud * ud) * b[QW_D2]) / (double)A.n_d : 0.0;
    const double tp = A.n_p ? ((up * up) * b[QW_P2]) / (double)A.n_p : 0.0;
    const double tc = c2 / (double)A.nz;
    q = (td + tp) + tc;
    if (q != q) q = __longlong_as_double(QF_INF_BITS);
  }
  b[QW_Q] = q; b[QW_C2] = c2; b[QW_NAN] = nan; b[QW_LAST_AP] = ap; b[QW_LAST_AD] = ad;
  const long long evals = qf_word(b, QW_EVALS) + 1;
  qf_set_word(b, QW_EVALS, evals);
  if (evals == 1 || q < b[QW_QBEST]) { b[QW_BEST] = sigma; b[QW_QBEST] = q; }      // the first of equal values stays
  long long phase = qf_word(b, QW_PHASE), steps = qf_word(b, QW_STEPS);
  double lo_ = b[QW_A], hi_ = b[QW_B];
  bool done = false, step = false;
  double next = sigma;
  if (phase == QP_FIRST) {
    b[QW_Q0] = q;
    next = qf_max(b[QW_LO], sigma * (1.0 - 1e-2));
    phase = QP_SECOND;
  } else if (phase == QP_SECOND) {
    if (q <= b[QW_Q0]) { lo_ = b[QW_LO]; hi_ = sigma; }
    else { lo_ = b[QW_SIGMA0]; hi_ = b[QW_HI]; }
    const double w = hi_ - lo_;
    if (w <= A.sigma_tol * hi_) {
      done = true;
    } else {
      const double gw = QF_GOLDEN * w;
      b[QW_C] = hi_ - gw;
      b[QW_D] = lo_ + gw;
      next = b[QW_C];
      phase = QP_LEFT;
    }
  } else if (phase == QP_LEFT) {
    b[QW_QC] = q;
    next = b[QW_D];
    phase = QP_RIGHT;
  } else if (phase == QP_NEW_LEFT) {
    b[QW_QC] = q;
    step = true;
  } else {      // QP_RIGHT, QP_NEW_RIGHT
    b[QW_QD] = q;
    step = true;
  }
  if (step) {
    if (steps >= A.max_steps) {
      done = true;
    } else {
      if (b[QW_QC] <= b[QW_QD]) {
        hi_ = b[QW_D];
        b[QW_D] = b[QW_C];
        b[QW_QD] = b[QW_QC];
        const double gw = QF_GOLDEN * (hi_ - lo_);
        b[QW_C] = hi_ - gw;
        next = b[QW_C];
        phase = QP_NEW_LEFT;
      } else {
        lo_ = b[QW_C];
        b[QW_C] = b[QW_D];
        b[QW_QC] = b[QW_QD];
        const double gw = QF_GOLDEN * (hi_ - lo_);
        b[QW_D] = lo_ + gw;
        next = b[QW_D];
        phase = QP_NEW_RIGHT;
      }
      ++steps;
      if (hi_ - lo_ <= A.sigma_tol * hi_) done = true;
    }
  }
  b[QW_A] = lo_; b[QW_B] = hi_;
  qf_set_word(b, QW_PHASE, phase);
  qf_set_word(b, QW_STEPS, steps);
  if (done) {
    qf_set_word(b, QW_STATUS, __double_as_longlong(b[QW_QBEST]) == QF_INF_BITS ? QF_UNUSABLE : QF_DONE);
  } else {
    b[QW_SIGMA] = next;
  }
  qf_set_word(b, QW_ALPHA_P, (long long)QF_ONE_BITS);
  qf_set_word(b, QW_ALPHA_D, (long long)QF_ONE_BITS);
}

extern "C" __global__ __launch_bounds__(256) void qf_value(const QfArgs A) {
  __shared__ double lds[16];      // 2 (NW + 1) + 1 doubles at least: the parked columns, the totals, the flag
  if (qf_word(A.qblk, QW_STATUS) != QF_SECTION) return;      // gated: before the first store
  const long long stride = (long long)gridDim.x * 256;
  const double t = qf_t(A.qblk, A.mu_ref);
  const double ap = A.qblk[QW_ALPHA_P], ad = A.qblk[QW_ALPHA_D];
  double v[2] = {0.0, 0.0};       // C2, the count of NaN products
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      if (f & 3) {
        const double x = A.x[i];
        const double tp = ap * qf_dir(A.sol0[i], A.sol1[i], t);
        if (f & 1) {
          const double u = ad * qf_dir(A.dzL0[i], A.dzL1[i], t);
          qf_product(v, x - A.xl[i], tp, false, A.zL[i], u);
        }
        if (f & 2) {
          const double u = ad * qf_dir(A.dzU0[i], A.dzU1[i], t);
          qf_product(v, A.xu[i] - x, tp, true, A.zU[i], u);
        }
      }
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (!(f & 4) && (f & 3)) {
        const double s = A.s[j];
        const double tp = ap * qf_dir(A.ds0[j], A.ds1[j], t);
        if (f & 1) {
          const double u = ad * qf_dir(A.dvL0[j], A.dvL1[j], t);
          qf_product(v, s - A.rl[j], tp, false, A.vL[j], u);
        }
        if (f & 2) {
          const double u = ad * qf_dir(A.dvU0[j], A.dvU1[j], t);
          qf_product(v, A.ru[j] - s, tp, true, A.vU[j], u);
        }
      }
    }
  }
  // every workgroup has read the block by now: the last arrival is the only writer of this launch
  iem_shared_park<2>(v, A.red, A.tab, (long long)blockIdx.x, lds);
  if (!iem_shared_last(A.red + 2 * A.n_wg, (long long)blockIdx.x, A.n_wg, lds + 15)) return;
  iem_shared_totals(2, A.red, A.tab, A.tab + 2, A.tab + 4, lds);
  if (threadIdx.x == 0) qf_section(A, lds[0], lds[1], ap, ad);
}

// a new solve: the section idle, every word zero (the blocks of the iem_mu and the iem_amu have resets of their own)
extern "C" __global__ __launch_bounds__(64) void qf_reset(const QfArgs A) {
  if (threadIdx.x < QW_WORDS) A.qblk[threadIdx.x] = 0.0;
}

// Ipopt's scaled optimality error from the twelve words (AmuTerms, amu_ec, amu_E of iem_amu_device.h, word for word)
struct QfTerms { double e_d, e_p, sc; double pmax, pmin; bool has_nz; };
__device__ __forceinline__ double qf_ec(const QfTerms &t, double mu) { return t.has_nz ? qf_max(t.pmax - mu, mu - t.pmin) / t.sc : 0.0; }
__device__ __forceinline__ double qf_E(const QfTerms &t, double mu) { return qf_max(qf_max(t.e_d, t.e_p), qf_ec(t, mu)); }

// the ring of references of the iem_amu block (amu_ring, amu_remember)
__device__ __forceinline__ long long qf_ring(const double *ablk) {
  const long long n = qf_word(ablk, QAW_NREFS);
  return n < 0 ? 0 : n > QF_REFS ? QF_REFS : n;
}
__device__ __forceinline__ void qf_remember(double *ablk, long long refs_max, double e0) {
  long long n = qf_ring(ablk);
  if (n >= refs_max) {
    for (long long i = 1; i < n; ++i) ablk[QAW_REF0 + i - 1] = ablk[QAW_REF0 + i];
    --n;
  }
  ablk[QAW_REF0 + n] = e0;
  qf_set_word(ablk, QAW_NREFS, n + 1);
}

extern "C" __global__ __launch_bounds__(64) void qf_update(const QfArgs A) {
  if (threadIdx.x != 0) return;
  double *blk = A.mblk, *ab = A.ablk;
  const double *qb = A.qblk;
  const double *w = A.w;
  const double s_max = A.s_max;
  const long long m = A.ncon, nz = A.nz, mnz = m + nz;
  const double sd = qf_max(s_max, (w[4] + w[5]) / (double)(mnz > 1 ? mnz : 1)) / s_max;
  QfTerms t;
  t.sc = qf_max(s_max, w[5] / (double)(nz > 1 ? nz : 1)) / s_max;
  t.e_d = qf_max(w[0], w[1]) / sd;
  t.e_p = m ? w[2] : 0.0;
  t.pmax = w[3]; t.pmin = w[8];
  t.has_nz = nz != 0;
  const double mu_old = blk[QMW_MU];
  double mu = mu_old;
  const double e0 = qf_E(t, 0.0), ec0 = qf_ec(t, 0.0);
  long long status, k = 0;
  const bool unusable = w[10] != 0.0 || e0 != e0 || qf_word(qb, QW_STATUS) != QF_DONE;      // a section that is not DONE
  if (unusable) {
    status = QF_MU_UNUSABLE;
  } else if (e0 <= A.tol) {
    status = QF_MU_CONVERGED;
  } else if (nz == 0) {
    status = QF_MU_ITERATING;
    mu = A.mu_min;
  } else {
    status = QF_MU_ITERATING;
    const double avg = w[9] / (double)nz;
    ab[QAW_AVG] = avg;
    double mu_hi = ab[QAW_MU_MAX];
    if (__double_as_longlong(mu_hi) == 0ll) {
      mu_hi = A.mu_max_fact * avg;
      ab[QAW_MU_MAX] = mu_hi;
    }
    const long long nref = qf_ring(ab);
    bool progress = nref < A.refs_max;
    if (!progress) {
      double worst = ab[QAW_REF0];
      for (long long i = 1; i < nref; ++i) worst = qf_max(worst, ab[QAW_REF0 + i]);
      progress = e0 <= A.red_fact * worst;
    }
    long long mode = qf_word(ab, QAW_MODE);
    if (mode == QF_FIXED) {
      if (progress) {
        mode = QF_FREE;
        qf_set_word(ab, QAW_TO_FREE, qf_word(ab, QAW_TO_FREE) + 1);
        qf_remember(ab, A.refs_max, e0);
      } else {
        while (mu > A.mu_floor && qf_E(t, mu) <= A.kappa_eps * mu && k < QF_MAX_DECREASES) {
          mu = qf_max(A.mu_floor, qf_min(A.kappa_mu * mu, mu * sqrt(mu)));
          ++k;
        }
      }
    } else {
      if (progress && !A.force_fixed) {
        qf_remember(ab, A.refs_max, e0);
      } else {
        mode = QF_FIXED;
        qf_set_word(ab, QAW_TO_FIXED, qf_word(ab, QAW_TO_FIXED) + 1);
        mu = qf_min(qf_max(A.init_factor * avg, A.mu_min), mu_hi);
      }
    }
    qf_set_word(ab, QAW_MODE, mode);
    if (mode == QF_FREE) {
      const double sigma = qb[QW_BEST];      // the evaluated sigma of least q
      const double mu_or = sigma * avg;
      ab[QAW_MU_ORACLE] = mu_or;
      ab[QAW_SIGMA] = sigma;
      ab[QAW_M_AFF] = qb[QW_QBEST];          // (the word of the probing oracle's m_aff: the least q)
      mu = qf_min(qf_max(mu_or, A.mu_min), mu_hi);
    }
  }
  const long long flags = qf_word(blk, QMW_FLAGS);
  if (__double_as_longlong(mu) != __double_as_longlong(mu_old)) {
    blk[QMW_MU] = mu;
    blk[QMW_TAU] = qf_max(A.tau_min, 1.0 - mu);
    blk[QMW_ZETA] = sqrt(mu);
    qf_set_word(blk, QMW_FLAGS, flags | 1ll);
    if (A.sctl) { A.sctl[11] = 0.0; A.sctl[12] = 0.0; }      // the filter count and the flags: what iem_search_reset clears
  } else {
    qf_set_word(blk, QMW_FLAGS, flags & ~1ll);
  }
  if (k > 0) qf_set_word(blk, QMW_DECREASES, qf_word(blk, QMW_DECREASES) + k);
  blk[QMW_E0] = e0;
  blk[QMW_EMU] = qf_E(t, mu);
  blk[QMW_ED] = t.e_d;
  blk[QMW_EP] = t.e_p;
  blk[QMW_EC0] = ec0;
  qf_set_word(blk, QMW_STATUS, status);
  qf_set_word(blk, QMW_UPDATES, qf_word(blk, QMW_UPDATES) + 1);
}
