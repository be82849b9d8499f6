// iem_mpc_device.h — the kernels of the iem_mpc object (include/iem.h): MEHROTRA'S CORRECTOR on the blocks of an iem_amu object — the
// two-column right-hand side whose second column carries the second-order term of the complementarity equations (mpc_terms: the
// target of a bound is mu − dgap_aff·dz_aff in the place of mu), the slack and bound-multiplier directions and the step lengths of
// the corrected solution (mpc_step), and the safeguard's decision with the copy over the first-order direction (mpc_select).  A code
// object of its own (no other source key knows of it), compiled with -ffp-contract=off behind the helpers of iem_device.h
// (everything in front of its own kernels, with IEM_TILE = 256): every line below is the order of operations of the contract in
// include/iem.h, each operation rounded once.
//
// NO FLOAT ATOMIC, no inline assembly and no scratch in this file.  The only atomic is the integer atomicMin of mpc_step on the bit
// pattern of a non-negative double — the scheme of barrier_step (csrc/iem_barrier_device.h): the waves' values meet in LDS first, at
// most ONE per workgroup and slot, and none where a relaxed look at the slot shows that it would not change it.  There is no sum.
//
// The grid of the barrier object: one thread takes the entries i, i + stride, ... of [0, nvar + ncon): i < nvar is variable i,
// otherwise row j = i − nvar; fx[i] bit 0 = lower bound present, bit 1 = upper; fc[j] the same for an inequality row's slack, bit 2 =
// equality row.  Nothing is read where no bound is present, nor on equality rows of the slack side; dy of the affine direction is
// never read.  mpc_reset: ONE workgroup of 64 threads.
//
// mu and tau: words 0 and 1 of the iem_mu block where A.mblk is not null (iem_mpc_bind_mu), the host's A.mu / A.tau otherwise — a
// branch every thread takes the same way.

#define MPC_ONE_BITS 0x3ff0000000000000ull   // 1.0

// the object's own block: words of 8 bytes
enum { MW_TAKEN, MW_N_TAKEN, MW_N_REFUSED, MW_PREDICTED, MW_AVG, MW_ALPHA_P, MW_ALPHA_D };
#define MPC_AW_AVG 9      // word 9 of the iem_amu block (AW_AVG of csrc/iem_amu_device.h)

struct MpcArgs {
  const double *xl, *xu, *rl, *ru, *ceq;          // the barrier object's relaxed bounds and the equality rows' right-hand side
  const unsigned char *fx, *fc;
  const double *x, *s, *y, *zL, *zU, *vL, *vU;    // the state
  const double *r, *c;                            // terms: sigma grad f + J'y (nvar), c(x) (ncon)
  const double *sol_a, *ds_a, *dzL_a, *dzU_a, *dvL_a, *dvU_a;      // the affine direction: sol_a = [dx; dy], dy never read
  const double *sol;                              // step, select: the corrected solution [dx; dy] (column 1 of the solve)
  double *ds, *dzL, *dzU, *dvL, *dvU;             // the corrected directions (step writes, select reads)
  double *rhs0, *rhs1;                            // terms: the two columns
  unsigned long long *alpha;                      // {alpha_primal, alpha_dual} of the corrected direction as bit patterns (step writes, select reads)
  const double *probe;                            // select: the four words of amu_probe on the corrected direction
  double *o_sol, *o_ds, *o_dzL, *o_dzU, *o_dvL, *o_dvU, *o_alpha;      // select: the first-order direction and its step lengths
  const double *mblk;                             // the iem_mu block {mu, tau, ...}, or null — then mu / tau below rule
  const double *ablk;                             // the iem_amu block (word 9: avg)
  double *blk;                                    // the object's own block
  double mu, tau, red_fact;
  long long nz;
  long long nvar, n;
};

__device__ __forceinline__ unsigned long long mpc_cand(double a) { return a > 0.0 ? (unsigned long long)__double_as_longlong(a) : 0ull; }
__device__ __forceinline__ unsigned long long mpc_umin(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ void mpc_set_word(double *blk, int w, long long v) { blk[w] = __longlong_as_double(v); }

// The two minima of the workgroup into their slots (bar_extremes<2, true> of csrc/iem_barrier_device.h): per wave by shuffles, across
// the waves through LDS, then thread s < 2 holds value s of the workgroup and issues ONE integer atomic — and none where a relaxed
// agent-scope look at the slot shows that it would not change it.
__device__ __forceinline__ void mpc_minima(unsigned long long (&v)[2], unsigned long long *slots, unsigned long long *lds) {
  constexpr int NW = IEM_TILE / IEM_WAVE;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    for (int o = 32; o > 0; o >>= 1) v[s] = mpc_umin(v[s], __shfl_xor(v[s], o, 64));
    if (iem_lane() == 0) lds[iem_wave() * 2 + s] = v[s];
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int s = (int)threadIdx.x;
    unsigned long long b = lds[s];
    for (int w = 1; w < NW; ++w) b = mpc_umin(b, lds[w * 2 + s]);
    const unsigned long long cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b < cur) atomicMin(slots + s, b);
  }
}

extern "C" __global__ __launch_bounds__(256) void mpc_terms(const MpcArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mblk ? A.mblk[0] : A.mu;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const bool hl = A.fx[i] & 1, hu = A.fx[i] & 2;
      double ml0 = 0.0, mu0 = 0.0, ml1 = 0.0, mu1 = 0.0;
      if (hl || hu) {
        const double x = A.x[i], da = A.sol_a[i];
        if (hl) { const double d = x - A.xl[i]; const double e = da * A.dzL_a[i]; const double m = mu - e; ml0 = mu / d; ml1 = m / d; }
        if (hu) { const double d = A.xu[i] - x; const double e = da * A.dzU_a[i]; const double m = mu + e; mu0 = mu / d; mu1 = m / d; }
      }
      const double r = A.r[i];
      const double gb0 = mu0 - ml0, gb1 = mu1 - ml1;
      A.rhs0[i] = -(r + gb0);
      A.rhs1[i] = -(r + gb1);
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (f & 4) {
        const double v = -(A.c[j] - A.ceq[j]);
        A.rhs0[i] = v;
        A.rhs1[i] = v;
        continue;
      }
      const double s = A.s[j];
      double sl = 0.0, su = 0.0, ml0 = 0.0, mu0 = 0.0, ml1 = 0.0, mu1 = 0.0;
      if (f & 3) {
        const double da = A.ds_a[j];
        if (f & 1) { const double g = s - A.rl[j]; const double e = da * A.dvL_a[j]; const double m = mu - e; sl = A.vL[j] / g; ml0 = mu / g; ml1 = m / g; }
        if (f & 2) { const double g = A.ru[j] - s; const double e = da * A.dvU_a[j]; const double m = mu + e; su = A.vU[j] / g; mu0 = mu / g; mu1 = m / g; }
      }
      const double sigs = sl + su, gs0 = mu0 - ml0, gs1 = mu1 - ml1;
      const double y = A.y[j];
      const double rs0 = gs0 - y, rs1 = gs1 - y, inv = 1.0 / sigs;
      const double cs = A.c[j] - s;
      A.rhs0[i] = -(cs + rs0 * inv);
      A.rhs1[i] = -(cs + rs1 * inv);
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void mpc_step(const MpcArgs A) {
  __shared__ unsigned long long lds[2 * (IEM_TILE / IEM_WAVE)];
  const long long stride = (long long)gridDim.x * 256;
  const double mu = A.mblk ? A.mblk[0] : A.mu, tau = A.mblk ? A.mblk[1] : A.tau;
  const double ntau = -tau;
  unsigned long long ap = MPC_ONE_BITS, ad = MPC_ONE_BITS;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const bool hl = A.fx[i] & 1, hu = A.fx[i] & 2;
      const double x = A.x[i], dx = A.sol[i];
      double dzl = 0.0, dzu = 0.0;
      if (dx != dx) ap = 0ull;      // a NaN in the direction: unusable, whatever the bounds
      if (hl) {
        const double d = x - A.xl[i], z = A.zL[i];
        const double e = A.sol_a[i] * A.dzL_a[i];
        const double m = mu - e;
        dzl = (m / d - z) - (z / d) * dx;
        if (dx < 0.0) ap = mpc_umin(ap, mpc_cand((ntau * d) / dx));
        if (dzl < 0.0) ad = mpc_umin(ad, mpc_cand((ntau * z) / dzl));
        if (dzl != dzl) ad = 0ull;
      }
      if (hu) {
        const double d = A.xu[i] - x, z = A.zU[i];
        const double e = A.sol_a[i] * A.dzU_a[i];
        const double m = mu + e;
        dzu = (m / d - z) + (z / d) * dx;
        if (dx > 0.0) ap = mpc_umin(ap, mpc_cand((tau * d) / dx));
        if (dzu < 0.0) ad = mpc_umin(ad, mpc_cand((ntau * z) / dzu));
        if (dzu != dzu) ad = 0ull;
      }
      A.dzL[i] = dzl;
      A.dzU[i] = dzu;
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (A.sol[i] != A.sol[i]) ap = 0ull;      // dy
      if (f & 4) continue;
      const bool gl = f & 1, gu = f & 2;
      const double s = A.s[j];
      double el = 0.0, eu = 0.0, vl = 0.0, vu = 0.0, sl = 0.0, su = 0.0, ml = 0.0, mu_u = 0.0;
      if (gl) { el = s - A.rl[j]; vl = A.vL[j]; sl = vl / el; const double e = A.ds_a[j] * A.dvL_a[j]; const double m = mu - e; ml = m / el; }
      if (gu) { eu = A.ru[j] - s; vu = A.vU[j]; su = vu / eu; const double e = A.ds_a[j] * A.dvU_a[j]; const double m = mu + e; mu_u = m / eu; }
      const double sigs = sl + su, gs = mu_u - ml;
      const double rs = gs - A.y[j];
      const double ds = (A.sol[i] - rs) / sigs;
      A.ds[j] = ds;
      if (ds != ds) ap = 0ull;
      double dvl = 0.0, dvu = 0.0;
      if (gl) {
        dvl = (ml - vl) - sl * ds;
        if (ds < 0.0) ap = mpc_umin(ap, mpc_cand((ntau * el) / ds));
        if (dvl < 0.0) ad = mpc_umin(ad, mpc_cand((ntau * vl) / dvl));
        if (dvl != dvl) ad = 0ull;
      }
      if (gu) {
        dvu = (mu_u - vu) + su * ds;
        if (ds > 0.0) ap = mpc_umin(ap, mpc_cand((tau * eu) / ds));
        if (dvu < 0.0) ad = mpc_umin(ad, mpc_cand((ntau * vu) / dvu));
        if (dvu != dvu) ad = 0ull;
      }
      A.dvL[j] = dvl;
      A.dvU[j] = dvu;
    }
  }
  unsigned long long a[2] = {ap, ad};      // the slots were seeded with the bits of 1.0 in front of the launch
  mpc_minima(a, A.alpha, lds);
}

// Every thread reads the same few words — none of which this launch writes — and decides the same way; refused, the call returns
// before its first store to a direction.  One thread of workgroup 0 writes the object's own block (which no other thread reads) and,
// taken, the two step lengths.
extern "C" __global__ __launch_bounds__(256) void mpc_select(const MpcArgs A) {
  const double q_sum = A.probe[0], q_nan = A.probe[1];
  const unsigned long long ap = A.alpha[0], ad = A.alpha[1];
  const double avg = A.ablk[MPC_AW_AVG];
  const double predicted = A.nz ? q_sum / (double)A.nz : 0.0;
  const double bound = A.red_fact * avg;
  const bool taken = A.nz != 0 && q_nan == 0.0 && ap != 0ull && ad != 0ull && predicted <= bound;      // a NaN compares false
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double *blk = A.blk;
    const long long n_taken = __double_as_longlong(blk[MW_N_TAKEN]) + (taken ? 1 : 0);
    const long long n_refused = __double_as_longlong(blk[MW_N_REFUSED]) + (taken ? 0 : 1);
    mpc_set_word(blk, MW_TAKEN, taken ? 1ll : 0ll);
    mpc_set_word(blk, MW_N_TAKEN, n_taken);
    mpc_set_word(blk, MW_N_REFUSED, n_refused);
    blk[MW_PREDICTED] = predicted;
    blk[MW_AVG] = avg;
    mpc_set_word(blk, MW_ALPHA_P, (long long)ap);
    mpc_set_word(blk, MW_ALPHA_D, (long long)ad);
    for (int w = MW_ALPHA_D + 1; w < 16; ++w) blk[w] = 0.0;
    if (taken) {
      mpc_set_word(A.o_alpha, 0, (long long)ap);
      mpc_set_word(A.o_alpha, 1, (long long)ad);
    }
  }
  if (!taken) return;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    A.o_sol[i] = A.sol[i];
    if (i < A.nvar) {
      A.o_dzL[i] = A.dzL[i];
      A.o_dzU[i] = A.dzU[i];
    } else {
      const long long j = i - A.nvar;
      if (A.fc[j] & 4) continue;
      A.o_ds[j] = A.ds[j];
      A.o_dvL[j] = A.dvL[j];
      A.o_dvU[j] = A.dvU[j];
    }
  }
}

// a new solve: the block zero
extern "C" __global__ __launch_bounds__(64) void mpc_reset(const MpcArgs A) {
  if (threadIdx.x < 16) A.blk[threadIdx.x] = 0.0;
}
