// iem_kkt_diag_device.h — the finishing kernels of the KKT object (iem_kkt_assemble* / iem_kkt_residual* / iem_kkt_solve_refined*):
// K = [W + diag(sigma) + delta_w I, J'; J, −diag(dcon + delta_c)]  with an optional PER-ROW diagonal dcon in the constraint block,
// its residual and its refinement over one or several columns.  A code object of its own (no other source key knows of it), compiled
// with -ffp-contract=off: every line below is the order of operations of the contract in include/iem.h.
//
//   kkt_gather_d:    the dense blocks from the COO values.  flat[dest[i]] = sum over k in [seg[i], seg[i + 1]) of the source perm[k]
//                    — an index into the virtual array
//                      hess values | jac values | (sigma + delta_w) per variable | per constraint row | 1.0 (the padding's unit diagonal)
//                    summed from 0.0 in the order of the segment.  The per-row source is −delta_c without dcon and
//                    −(dcon[row] + delta_c) with it — one rounded add, then the negation, so that dcon ≡ d, delta_c = 0 gives the
//                    bits of delta_c = d.
//   kkt_residual_dm: entries x columns (blockIdx.y = column u, at base + u·ld).  p = K0·sol from iem_kktprod, then per entry
//                      i <  nvar:  r = rhs − (p + ((sigma ? sigma[i] : 0) + delta_w)·sol)
//                      i >= nvar:  d = dcon ? dcon[i − nvar] + delta_c : delta_c,   r = rhs − (p − d·sol)
//                    and, where asked for, max |r| of the column into norms[u]: the bit pattern of a non-negative double orders as
//                    an unsigned 64-bit integer (a NaN's lies above every finite one), so the maximum is taken on the patterns —
//                    per lane, across the wave by shuffles, across waves by ONE integer atomicMax per wave.  No float atomic, no order
//                    dependence: the result is bitwise reproducible.  norms is zeroed by the runtime in front of the launch.
//   kkt_axpy_m:      sol[u·ld_s + i] = sol[u·ld_s + i] + d[u·ld_d + i]  (one rounded add per entry)
//
// One thread takes the entries i, i + stride, ... of its column: plain vector loads and stores.

struct KktGatherDArgs {
  double *flat;
  const long long *dest;
  const unsigned *seg, *perm;
  const double *hess, *jac, *sigma, *dcon;   // sigma: nvar entries or null;  dcon: ncon entries or null
  double dw, dc;
  long long n_dest, n_h, n_j, n_var, n_con;
};

extern "C" __global__ __launch_bounds__(256) void kkt_gather_d(const KktGatherDArgs A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_dest) return;
  double acc = 0.0;
  for (unsigned k = A.seg[i]; k < A.seg[i + 1]; ++k) {
    long long s = A.perm[k];
    double v;
    if (s < A.n_h) v = A.hess[s];
    else if ((s -= A.n_h) < A.n_j) v = A.jac[s];
    else if ((s -= A.n_j) < A.n_var) v = (A.sigma ? A.sigma[s] : 0.0) + A.dw;
    else if ((s -= A.n_var) < A.n_con) v = A.dcon ? -(A.dcon[s] + A.dc) : -A.dc;
    else v = 1.0;
    acc += v;
  }
  A.flat[A.dest[i]] = acc;
}

struct KktResidualDmArgs {
  const double *p, *rhs, *sol, *sigma, *dcon;   // sigma: nvar entries or null;  dcon: ncon entries or null
  double *r;
  unsigned long long *norms;                    // one per column, or null: no norms
  double dw, dc;
  long long nvar, n;                            // n = nvar + ncon
  long long ld_p, ld_rhs, ld_sol, ld_r;
};

extern "C" __global__ __launch_bounds__(256) void kkt_residual_dm(const KktResidualDmArgs A) {
  const long long u = blockIdx.y, stride = (long long)gridDim.x * 256;
  const double *p = A.p + u * A.ld_p, *rhs = A.rhs + u * A.ld_rhs, *sol = A.sol + u * A.ld_sol;
  double *out = A.r + u * A.ld_r;
  unsigned long long best = 0ull;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    const double s = sol[i];
    double t;
    if (i < A.nvar) {
      const double d = (A.sigma ? A.sigma[i] : 0.0) + A.dw;
      t = p[i] + d * s;
    } else {
      const double d = A.dcon ? A.dcon[i - A.nvar] + A.dc : A.dc;
      t = p[i] - d * s;
    }
    const double r = rhs[i] - t;
    out[i] = r;
    const unsigned long long b = (unsigned long long)__double_as_longlong(r) & 0x7fffffffffffffffull;   // |r|
    best = b > best ? b : best;
  }
  if (!A.norms) return;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if ((threadIdx.x & 63) == 0 && best) atomicMax(A.norms + u, best);
}

struct KktAxpyMArgs {
  double *sol;
  const double *d;
  long long n, ld_s, ld_d;
};

extern "C" __global__ __launch_bounds__(256) void kkt_axpy_m(const KktAxpyMArgs A) {
  const long long u = blockIdx.y, stride = (long long)gridDim.x * 256;
  double *sol = A.sol + u * A.ld_s;
  const double *d = A.d + u * A.ld_d;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) sol[i] = sol[i] + d[i];
}
