// iem_amu_device.h — the kernels of the iem_amu object (include/iem.h): an ADAPTIVE barrier parameter on the block of an iem_mu
// object — the probing oracle's look along the affine-scaling direction (amu_probe: the complementarity the step (alpha_p, alpha_d)
// would leave behind), and the rule (amu_update): Ipopt's free / fixed modes with the kkt-error progress test on a ring of at most
// four references, the probing and the LOQO oracle in free mode, the monotone loop of mu_update in fixed mode.  A code object of its
// own (no other source key knows of it), compiled with -ffp-contract=off behind the helpers of iem_device.h (everything in front of
// its own kernels, with IEM_TILE = 256): every line below is the order of operations of the contract in include/iem.h, each
// operation rounded once.
//
// NO FLOAT ATOMIC, no inline assembly and no scratch in this file.  The two sums of amu_probe go through iem_shared_park /
// iem_shared_last / iem_shared_totals of iem_device.h as they stand: a lane adds its entries in index order, every workgroup parks
// its values, the workgroup that arrives last totals each column in a fixed order — the order of mu_error's word 9, so with zero
// directions and alpha = (1, 1) word 0 carries that word's bits.  No seed: all four words are written by the last arrival.
//
// amu_probe: the grid of the barrier object — one thread takes the entries i, i + stride, ... of [0, nvar + ncon): i < nvar is
// variable i, otherwise row j = i − nvar; flags as in mu_error (fx / fc bit 0 = lower bound present, bit 1 = upper, fc bit 2 =
// equality row).  Nothing is read where no bound is present.  amu_update, amu_reset: ONE workgroup of 64 threads, one thread decides.

#define AMU_ITERATING 0ll
#define AMU_CONVERGED 1ll
#define AMU_UNUSABLE 2ll
#define AMU_FREE 0ll
#define AMU_FIXED 1ll
#define AMU_PROBING 0ll
#define AMU_LOQO 1ll
#define AMU_MAX_DECREASES 64
#define AMU_REFS 4

// the iem_mu block (the words amu_update writes as mu_update does) and the object's own block: words of 8 bytes
enum { AMW_MU, AMW_TAU, AMW_ZETA, AMW_E0, AMW_EMU, AMW_ED, AMW_EP, AMW_EC0, AMW_STATUS, AMW_FLAGS, AMW_DECREASES, AMW_UPDATES };
enum { AW_MODE, AW_MU_MAX, AW_NREFS, AW_REF0, AW_MU_ORACLE = 7, AW_SIGMA, AW_AVG, AW_M_AFF, AW_TO_FIXED, AW_TO_FREE, AW_ORACLE };

struct AmuArgs {
  const double *xl, *xu, *rl, *ru;                // the barrier object's relaxed bounds
  const unsigned char *fx, *fc;
  const double *x, *s, *zL, *zU, *vL, *vU;        // the state
  const double *sol, *ds, *dzL, *dzU, *dvL, *dvU; // the affine direction: sol = [dx; dy]
  const double *alpha;                            // amu_probe: (alpha_p, alpha_d) of the affine step
  double *out;                                    // amu_probe: the four words
  const double *w;                                // amu_update: the twelve words of mu_error
  const double *probe;                            // amu_update: the four words of amu_probe, or null (LOQO)
  double *mblk;                                   // the iem_mu block
  double *ablk;                                   // the object's own block
  double *sctl;                                   // amu_update: the control block of a search whose filter a change of mu empties, or null
  double *red;                                    // 2 n_wg parked values, then the ticket words (the object's own)
  const long long *tab;                           // offs[2] | first[2] | count[2] of iem_shared_totals
  double kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max;      // of the iem_mu object
  double sigma_max, mu_min, mu_max_fact, init_factor, red_fact;
  long long refs_max, oracle, force_fixed;
  long long ncon, nz;
  long long nvar, n, n_wg;
};

// np.maximum / np.minimum: a NaN in either operand gives a NaN (mu_max / mu_min of iem_mu_device.h)
__device__ __forceinline__ double amu_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double amu_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ long long amu_word(const double *blk, int w) { return __double_as_longlong(blk[w]); }
__device__ __forceinline__ void amu_set_word(double *blk, int w, long long v) { blk[w] = __longlong_as_double(v); }

// one present bound: the product the step would leave, into the sum and the count of NaNs
struct AmuSums { double sum, nan; };
__device__ __forceinline__ void amu_product(AmuSums &q, double gap, double t, bool upper, double z, double u) {
  const double g = upper ? gap - t : gap + t;
  const double w = z + u;
  const double p = g * w;
  if (p != p) q.nan += 1.0;
  q.sum += p;
}

extern "C" __global__ __launch_bounds__(256) void amu_probe(const AmuArgs A) {
  __shared__ double lds[16];      // 2 (NW + 1) + 1 doubles at least: the parked columns, the totals, the flag
  const long long stride = (long long)gridDim.x * 256;
  const double ap = A.alpha[0], ad = A.alpha[1];
  AmuSums q = {0.0, 0.0};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      if (f & 3) {
        const double x = A.x[i];
        const double t = ap * A.sol[i];
        if (f & 1) {
          const double u = ad * A.dzL[i];
          amu_product(q, x - A.xl[i], t, false, A.zL[i], u);
        }
        if (f & 2) {
          const double u = ad * A.dzU[i];
          amu_product(q, A.xu[i] - x, t, true, A.zU[i], u);
        }
      }
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (!(f & 4) && (f & 3)) {
        const double s = A.s[j];
        const double t = ap * A.ds[j];
        if (f & 1) {
          const double u = ad * A.dvL[j];
          amu_product(q, s - A.rl[j], t, false, A.vL[j], u);
        }
        if (f & 2) {
          const double u = ad * A.dvU[j];
          amu_product(q, A.ru[j] - s, t, true, A.vU[j], u);
        }
      }
    }
  }
  const double cols[2] = {q.sum, q.nan};
  iem_shared_park<2>(cols, A.red, A.tab, (long long)blockIdx.x, lds);
  if (!iem_shared_last(A.red + 2 * A.n_wg, (long long)blockIdx.x, A.n_wg, lds + 15)) return;
  iem_shared_totals(2, A.red, A.tab, A.tab + 2, A.tab + 4, lds);
  if (threadIdx.x < 2) A.out[threadIdx.x] = lds[threadIdx.x];
  if (threadIdx.x == 2) A.out[2] = ap;
  if (threadIdx.x == 3) A.out[3] = ad;
}

// a new solve: mode FREE, the ring empty, mu_max unset, the oracle's words and the counters zero; word 13 names the oracle
extern "C" __global__ __launch_bounds__(64) void amu_reset(const AmuArgs A) {
  if (threadIdx.x >= 16) return;
  const int w = (int)threadIdx.x;
  if (w == AW_ORACLE) amu_set_word(A.ablk, w, A.oracle);
  else A.ablk[w] = 0.0;
}

// Ipopt's scaled optimality error from the twelve words (MuTerms, mu_ec, mu_E of iem_mu_device.h, word for word)
struct AmuTerms { double e_d, e_p, sc; double pmax, pmin; bool has_nz; };
__device__ __forceinline__ double amu_ec(const AmuTerms &t, double mu) { return t.has_nz ? amu_max(t.pmax - mu, mu - t.pmin) / t.sc : 0.0; }
__device__ __forceinline__ double amu_E(const AmuTerms &t, double mu) { return amu_max(amu_max(t.e_d, t.e_p), amu_ec(t, mu)); }

// the ring of references, oldest first: at refs_max the oldest leaves (a count outside 0..4 cannot come from these kernels; a block
// written by a host is read as holding at most four)
__device__ __forceinline__ long long amu_ring(const double *ablk) {
  const long long n = amu_word(ablk, AW_NREFS);
  return n < 0 ? 0 : n > AMU_REFS ? AMU_REFS : n;
}
__device__ __forceinline__ void amu_remember(double *ablk, long long refs_max, double e0) {
  long long n = amu_ring(ablk);
  if (n >= refs_max) {
    for (long long i = 1; i < n; ++i) ablk[AW_REF0 + i - 1] = ablk[AW_REF0 + i];
    --n;
  }
  ablk[AW_REF0 + n] = e0;
  amu_set_word(ablk, AW_NREFS, n + 1);
}

extern "C" __global__ __launch_bounds__(64) void amu_update(const AmuArgs A) {
  if (threadIdx.x != 0) return;
  double *blk = A.mblk, *ab = A.ablk;
  const double *w = A.w;
  const double s_max = A.s_max;
  const long long m = A.ncon, nz = A.nz, mnz = m + nz;
  const double sd = amu_max(s_max, (w[4] + w[5]) / (double)(mnz > 1 ? mnz : 1)) / s_max;
  AmuTerms t;
  t.sc = amu_max(s_max, w[5] / (double)(nz > 1 ? nz : 1)) / s_max;
  t.e_d = amu_max(w[0], w[1]) / sd;
  t.e_p = m ? w[2] : 0.0;
  t.pmax = w[3]; t.pmin = w[8];
  t.has_nz = nz != 0;
  const double mu_old = blk[AMW_MU];
  double mu = mu_old;
  const double e0 = amu_E(t, 0.0), ec0 = amu_ec(t, 0.0);
  const bool probing = A.oracle == AMU_PROBING;
  long long status, k = 0;
  bool unusable = w[10] != 0.0 || e0 != e0;
  if (probing) unusable = unusable || A.probe[1] != 0.0 || __double_as_longlong(A.probe[2]) == 0ll || __double_as_longlong(A.probe[3]) == 0ll;
  if (unusable) {
    status = AMU_UNUSABLE;
  } else if (e0 <= A.tol) {
    status = AMU_CONVERGED;
  } else if (nz == 0) {
    status = AMU_ITERATING;
    mu = A.mu_min;
  } else {
    status = AMU_ITERATING;
    const double avg = w[9] / (double)nz;
    ab[AW_AVG] = avg;
    double mu_hi = ab[AW_MU_MAX];
    if (__double_as_longlong(mu_hi) == 0ll) {
      mu_hi = A.mu_max_fact * avg;
      ab[AW_MU_MAX] = mu_hi;
    }
    const long long nref = amu_ring(ab);
    bool progress = nref < A.refs_max;
    if (!progress) {
      double worst = ab[AW_REF0];
      for (long long i = 1; i < nref; ++i) worst = amu_max(worst, ab[AW_REF0 + i]);
      progress = e0 <= A.red_fact * worst;
    }
    long long mode = amu_word(ab, AW_MODE);
    if (mode == AMU_FIXED) {
      if (progress) {
        mode = AMU_FREE;
        amu_set_word(ab, AW_TO_FREE, amu_word(ab, AW_TO_FREE) + 1);
        amu_remember(ab, A.refs_max, e0);
      } else {
        while (mu > A.mu_floor && amu_E(t, mu) <= A.kappa_eps * mu && k < AMU_MAX_DECREASES) {
          mu = amu_max(A.mu_floor, amu_min(A.kappa_mu * mu, mu * sqrt(mu)));
          ++k;
        }
      }
    } else {
      if (progress && !A.force_fixed) {
        amu_remember(ab, A.refs_max, e0);
      } else {
        mode = AMU_FIXED;
        amu_set_word(ab, AW_TO_FIXED, amu_word(ab, AW_TO_FIXED) + 1);
        mu = amu_min(amu_max(A.init_factor * avg, A.mu_min), mu_hi);
      }
    }
    amu_set_word(ab, AW_MODE, mode);
    if (mode == AMU_FREE) {
      double sigma, m_aff = 0.0;
      if (probing) {
        m_aff = A.probe[0] / (double)nz;
        const double q = m_aff / avg;
        sigma = amu_min((q * q) * q, A.sigma_max);
      } else {
        const double xi = w[8] / avg;
        const double f = (0.05 * (1.0 - xi)) / xi;
        const double c = amu_min(f, 2.0);
        sigma = 0.1 * ((c * c) * c);
      }
      const double mu_or = sigma * avg;
      ab[AW_MU_ORACLE] = mu_or;
      ab[AW_SIGMA] = sigma;
      ab[AW_M_AFF] = m_aff;
      mu = amu_min(amu_max(mu_or, A.mu_min), mu_hi);
    }
  }
  const long long flags = amu_word(blk, AMW_FLAGS);
  if (__double_as_longlong(mu) != __double_as_longlong(mu_old)) {
    blk[AMW_MU] = mu;
    blk[AMW_TAU] = amu_max(A.tau_min, 1.0 - mu);
    blk[AMW_ZETA] = sqrt(mu);
    amu_set_word(blk, AMW_FLAGS, flags | 1ll);
    if (A.sctl) { A.sctl[11] = 0.0; A.sctl[12] = 0.0; }      // the filter count and the flags: what iem_search_reset clears
  } else {
    amu_set_word(blk, AMW_FLAGS, flags & ~1ll);
  }
  if (k > 0) amu_set_word(blk, AMW_DECREASES, amu_word(blk, AMW_DECREASES) + k);
  blk[AMW_E0] = e0;
  blk[AMW_EMU] = amu_E(t, mu);
  blk[AMW_ED] = t.e_d;
  blk[AMW_EP] = t.e_p;
  blk[AMW_EC0] = ec0;
  amu_set_word(blk, AMW_STATUS, status);
  amu_set_word(blk, AMW_UPDATES, amu_word(blk, AMW_UPDATES) + 1);
}
