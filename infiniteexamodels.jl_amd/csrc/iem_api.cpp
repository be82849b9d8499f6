// iem_api.cpp — libiem_hip.so: C-ABI (include/iem.h) over the generated gfx950 kernels.
//
// Host side of the drop-in boundary: parses the transcribed model, generates and loads
// its fused kernels (code-object cache → hiprtc on a miss), keeps θ / item-data arrays
// resident in HBM, and enqueues one launch per support grid for each NLPModels call.
// There is NO CPU evaluation path in this library: without a HIP device iem_create
// fails with IEM_E_NODEVICE.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/iem.h"
#include "iem_codegen.hpp"
#include "iem_kkt_host.hpp"
#include <memory>
#include "iem_model.hpp"
#include "iem_shard.hpp"

static const char *kDeviceHeader =
#include "iem_device_h.inc"
    ;
static const char *kHalo2Header =   // the two-way halo exchange: only in the source of a two-sided shard (Options::two_sided)
#include "iem_halo2_device_h.inc"
    ;
static const char *kKktSource =
#include "iem_kkt_device_h.inc"
    ;
static const char *kKktManySource =   // the multi-column solve kernels, behind the single-column ones in every chain KKT code object
#include "iem_kkt_many_device_h.inc"
    ;
static const char *kKktDiagSource =       // the KKT object's gather, residual and add over one or several columns: a code object of its own
#include "iem_kkt_diag_device_h.inc"
    ;
static const char *kKktBorderSource =     // the dense border on the device (kkt_border_ldl / kkt_border_solve): a code object of its own
#include "iem_kkt_border_device_h.inc"
    ;
static const char *kBarrierSource =       // the interior-point barrier layer (iem_barrier_*): a code object of its own, behind the helpers of the device header (everything in front of its own kernels)
#include "iem_barrier_device_h.inc"
    ;
static const char *kSearchSource =        // the filter line search (iem_search_*): a code object of its own, behind the same helpers — not a row of kFixed
#include "iem_search_device_h.inc"
    ;
static const char *kSocSource =           // the second-order correction of the search (iem_soc_*): a code object of its own, behind no helpers — not a row of kFixed
#include "iem_soc_device_h.inc"
    ;
static const char *kRestoSource =         // the feasibility restoration phase (iem_resto_*): a code object of its own, behind the helpers of the device header — not a row of kFixed
#include "iem_resto_device_h.inc"
    ;
static const char *kMuSource =            // the barrier parameter (iem_mu_*): a code object of its own, behind the helpers of the device header — not a row of kFixed
#include "iem_mu_device_h.inc"
    ;
static const char *kAmuSource =           // the adaptive barrier parameter (iem_amu_*): a code object of its own, behind the helpers of the device header — not a row of kFixed
#include "iem_amu_device_h.inc"
    ;
static const char *kQfSource =            // the quality-function oracle (iem_qf_*): a code object of its own, behind the helpers of the device header — not a row of kFixed
#include "iem_qf_device_h.inc"
    ;
static const char *kMpcSource =           // Mehrotra's corrector (iem_mpc_*): a code object of its own, behind the helpers of the device header — not a row of kFixed
#include "iem_mpc_device_h.inc"
    ;
static const char *kInitSource =          // the starting point (iem_init_*): a code object of its own, behind the helpers of the device header — not a row of kFixed
#include "iem_init_device_h.inc"
    ;
static const char *kConvSource =          // the stopping test and the kept iterate (iem_conv_*): a code object of its own, behind the helpers of the device header — not a row of kFixed
#include "iem_conv_device_h.inc"
    ;
static const char *kRmuSource =           // the restoration phase's barrier parameter (iem_rmu_*): a code object of its own, behind the helpers of the device header — not a row of kFixed
#include "iem_rmu_device_h.inc"
    ;

namespace {

thread_local std::string g_err;
iem::Options g_opt;

int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail(IEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                   \
  } while (0)

// Entry points run on the handle's device whatever the calling thread's current device is.
struct DevGuard {
  int prev = -1;
  bool switched = false;
  explicit DevGuard(int d) {
    if (hipGetDevice(&prev) == hipSuccess && prev != d) switched = hipSetDevice(d) == hipSuccess;
  }
  ~DevGuard() { if (switched) hipSetDevice(prev); }
};

int g_opt_poll_obj = 1;   // iem_set_option("poll_obj", 0): iem_obj always synchronises the stream

std::string contract_flag(const iem::Options &o) { return o.fp_contract ? "-ffp-contract=fast" : "-ffp-contract=off"; }

// The head of every source: the first line carries the compile flags (`contract`: off / fast) so that an offline build
// (lib.precompile_source) and the hiprtc path compile the same key with the same options
std::string source_prelude(const std::string &contract) {
  return "// iem-flags: -O3 -ffp-contract=" + contract + " -std=c++17\n#ifndef __HIPCC_RTC__\n#include <hip/hip_runtime.h>\n#endif\n";
}

std::string full_source(const iem::Program &p, const iem::Options &o) {
  std::string s = source_prelude(o.fp_contract ? "fast" : "off");
  s += std::string("#define IEM_NT ") + (o.nt_stores ? "1" : "0") + "\n";
  s += "#define IEM_TILE " + std::to_string(p.block) + "\n";
  s += std::string("#define IEM_WIDE_STORES ") + (o.wide_stores ? "1" : "0") + "\n";
  if (o.flush32 != 2) s += "#define IEM_FLUSH32 " + std::to_string(o.flush32) + "\n";
  if (o.ablate) s += "#define IEM_ABLATE " + std::to_string(o.ablate & 1) + "  // timing experiment, results are wrong\n";
  // A program whose kernels all use one workgroup size sees the device header as it is.  Otherwise (jac_coord! /
  // hess_coord! of a large grid run wider tiles than the rest) the header's tile-dependent region is repeated per size,
  // each copy in a namespace iem_t<size> — the generator wraps the kernels of that size in the same namespace.
  std::vector<int> tiles;
  for (const iem::KernelDesc &kd : p.kernels)
    if (std::find(tiles.begin(), tiles.end(), kd.block) == tiles.end()) tiles.push_back(kd.block);
  std::sort(tiles.begin(), tiles.end());
  if (tiles.size() <= 1) {
    s += kDeviceHeader;
  } else {
    const std::string hdr(kDeviceHeader);
    const size_t a = hdr.find("// IEM-TILE-REGION-BEGIN"), b = hdr.find("// IEM-TILE-REGION-END");
    if (a == std::string::npos || b == std::string::npos || b < a) throw std::runtime_error("internal: device header without tile-region markers");
    s += hdr.substr(0, a);
    for (int t : tiles)
      s += "#undef IEM_TILE\n#define IEM_TILE " + std::to_string(t) + "\nnamespace iem_t" + std::to_string(t) + " {\n" + hdr.substr(a, b - a) + "}  // namespace iem_t" +
           std::to_string(t) + "\n";
    s += "#undef IEM_TILE\n#define IEM_TILE " + std::to_string(p.block) + "\n";
    s += hdr.substr(b);
  }
  if (o.two_sided) s += std::string("\n") + kHalo2Header;
  s += "\n";
  s += p.source;
  return s;
}

// The hand-written code objects whose source does not depend on a shape: one row of kFixed each — the name iem_fixed_source
// lists it under, the embedded text, whether the text sits behind the device header's helpers (everything in front of the
// header's own kernels), and its kernels in slot order (the enum beside the row names the slots).  A handle loads one at the
// first call that needs it (fixed_object); build() compiles every row offline.
enum Fixed { F_KDIAG, F_KBORDER, F_BARRIER, F_COUNT };
constexpr int kFixedSlots = 6;
enum { KDIAG_GATHER, KDIAG_RESIDUAL, KDIAG_AXPY };
enum { KBORDER_LDL, KBORDER_SOLVE, KBORDER_COLSUM, KBORDER_INERTIA };
enum { BAR_START, BAR_TERMS, BAR_STEP, BAR_UPDATE, BAR_ERROR, BAR_MERIT };
const struct FixedRow { const char *name, *text; bool behind_helpers; const char *kernels[kFixedSlots]; } kFixed[F_COUNT] = {
    {"kkt_diag", kKktDiagSource, false, {"kkt_gather_d", "kkt_residual_dm", "kkt_axpy_m"}},      // iem_kkt_assemble* / iem_kkt_residual* / iem_kkt_solve_refined*
    {"kkt_border", kKktBorderSource, false, {"kkt_border_ldl", "kkt_border_solve", "kkt_border_colsum", "kkt_border_inertia"}},      // iem_kkt_border_* / iem_kkt_set_border
    {"barrier", kBarrierSource, true, {"barrier_start", "barrier_terms", "barrier_step", "barrier_update", "barrier_error", "barrier_merit"}},      // iem_barrier_*
};

// the source of a hand-written code object: the prelude, the helpers of the device header where the text sits behind them, the text
int object_source(const char *text, bool behind_helpers, std::string &s) {
  s = source_prelude("off");
  if (behind_helpers) {
    const std::string hdr(kDeviceHeader);
    const size_t b = hdr.find("// IEM-TILE-REGION-END");
    if (b == std::string::npos) return fail(IEM_E_COMPILE, "internal: device header without tile-region markers");
    s += "#define IEM_TILE 256\n" + hdr.substr(0, b) + "#endif  // IEM_DEVICE_H (its kernels are not part of this code object)\n\n";
  }
  s += text;
  return IEM_OK;
}
int fixed_source(Fixed f, std::string &s) { return object_source(kFixed[f].text, kFixed[f].behind_helpers, s); }

// what every *_source entry point returns: a malloc'ed copy of the text and its cache key
int emit_out(const std::string &s, char **out_src, uint64_t *out_key) {
  if (out_src) {
    *out_src = (char *)std::malloc(s.size() + 1);
    std::memcpy(*out_src, s.c_str(), s.size() + 1);
  }
  if (out_key) *out_key = iem::fnv1a64(s);
  return IEM_OK;
}
int fixed_source_out(Fixed f, char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = fixed_source(f, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

std::string lib_dir() {
  Dl_info info;
  if (dladdr((void *)&iem_version, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    size_t k = p.find_last_of('/');
    if (k != std::string::npos) return p.substr(0, k);
  }
  return ".";
}

std::string cache_dir() {
  const char *e = std::getenv("IEM_KERNEL_CACHE");
  if (e && *e) return e;
  return lib_dir() + "/kernels";   // next to libiem_hip.so: where lib.precompile / build() put the offline-built objects
}

std::string key_hex(uint64_t k) {
  char b[32];
  std::snprintf(b, sizeof b, "%016llx", (unsigned long long)k);
  return b;
}

bool read_file(const std::string &path, std::vector<char> &out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  f.seekg(0, std::ios::end);
  std::streamsize n = f.tellg();
  if (n <= 0) return false;
  f.seekg(0);
  out.resize((size_t)n);
  return (bool)f.read(out.data(), n);
}

}  // namespace

// A generated program as loaded for launching: its module and kernel functions and, per kernel, the argument block
// (LaunchHead, then the tables) with the device copy of the tables that do not fit it.  launchable[kind]: the kernels of
// the kind that have work (n_blocks > 0), in program order — what launch_kind launches.
struct CodeObject {
  iem::Program prog;
  hipModule_t mod = nullptr;
  std::vector<hipFunction_t> fns;
  std::vector<std::vector<uint64_t>> argbuf;
  std::vector<void *> d_tables;
  std::vector<int> launchable[iem::KK_LAST + 1];
};

// Everything a program owns on a handle: the code object and the device buffers its kernels and their follow-ups use.  The
// model's own program, the tuner's second object and every derived program (kDerived) are instances; release_program
// frees one, whatever of it exists.
struct LoadedProgram : CodeObject {
  double *d_red[iem::KK_COUNT] = {};         // per scatter kind: parked shared-entry values + tickets (iem_shared_*)
  long long *d_axis[iem::KK_COUNT] = {};     // per scatter kind: table of its axis sums (iem_axis_sum_kernel)
  long long *d_gather[iem::KK_COUNT] = {};   // per scatter kind: dest | seg | perm of its plan-driven gather (iem_gather_sum_kernel)
  std::vector<std::pair<int64_t, int64_t>> zero_ranges[iem::KK_COUNT];  // per scatter kind: [lo, hi) of the output its kernels do not overwrite
  double *d_partials = nullptr;              // the partials and ticket words of its objective kernels (programs that have some)
  // a derived program: set up by its first call or its prepare call; a failure that is remembered is reported by every later call
  bool tried = false;
  int rc = IEM_OK;
  std::string err;
};

// The derived programs of a handle, in the order iem_kernel_info lists their kernels behind the model's own (kDerived has
// a row for each)
enum Derived { D_PAR, D_ADJ, D_TH2, D_PC, D_LAG, D_SCL, D_KKT, D_SPH, D_COUNT };

struct iem_model {
  iem::Model model;
  LoadedProgram code;   // the model's program
  iem::Options opt;     // this handle's generator options (process defaults + iem_create_opts overrides)
  int poll_obj = 1;
  int device = 0;
  hipStream_t stream = nullptr;
  hipFunction_t fn_struct = nullptr, fn_csr = nullptr, fn_csr32 = nullptr, fn_axis = nullptr, fn_spmv = nullptr, fn_spmv_long = nullptr;
  hipFunction_t fn_gather = nullptr;
  double *d_theta = nullptr;
  // Second code object of jac_coord!/hess_coord! with a larger LDS staging batch (lds_slots = 48: one 96-KB
  // workgroup per CU, a third of the concurrently open store streams) and the tuner that picks, per kind and
  // per OUTPUT BUFFER, whichever of the two is faster there — how a COO buffer's physical pages fall onto the HBM
  // channels decides that, and both variants write identical bytes, so the first twenty calls into a
  // buffer run ten with one, ten with the other, under HIP events, and every call is a valid evaluation.
#define IEM_TUNE_CALLS 20   // measured calls per output buffer: a block of ten per variant
  LoadedProgram alt;   // loaded (alt.mod set) only where the tuner runs; jac_coord! / hess_coord! only, so it owns no buffer
  struct Tune {
    const void *out = nullptr;   // the buffer the decision belongs to
    int calls = 0, choice = -1;  // choice: -1 undecided, 0 default, 1 alt
    hipEvent_t ev[IEM_TUNE_CALLS][2] = {};
    bool have_events = false;
  };
  struct TuneSet {               // decisions for the last four output buffers of a kind (a solver alternates between few)
    Tune slot[4];
    int next = 0;
  } tune[2];   // [0] jac_coord!, [1] hess_coord!
  // multi-GPU (iem_create_sharded): what was cut, and the mailbox the peers push into
  bool sharded = false;
  iem::ShardInfo shard;
  hipFunction_t fn_halo = nullptr, fn_reduce = nullptr, fn_fold = nullptr;   // (a two-sided shard: the two-way kernels of iem_halo2_device.h)
  unsigned long long *mailbox = nullptr;   // device memory, exported through HIP IPC
  size_t mailbox_words = 0;
  int mailbox_kind = 0;   // 0 none yet, 1 uncached (fine-grained) device memory, 2 plain hipMalloc
  bool connected = false;
  std::vector<unsigned long long *> peers; // peers[r]: rank r's mailbox as mapped here (peers[rank] = mailbox)
  std::vector<void *> ipc_opened;          // what hipIpcCloseMemHandle must release
  unsigned long long **d_peers = nullptr;
  long long *d_halo_src = nullptr, *d_halo_dst = nullptr, *d_shared = nullptr;
  long long *d_halo_src_l = nullptr, *d_halo_dst_r = nullptr;   // second direction: my first owned supports (go left), my back halo entries
  int64_t n_shared = 0;
  double *h_obj = nullptr;   // pinned + mapped host scalar
  double *d_hobj = nullptr;  // its device address
  bool obj_armed = false;    // iem_obj_begin launched, iem_obj_end not yet called
  // a mailbox wait that timed out (iem_device.h: IemCommErr) also lands here — mapped pinned host memory the host
  // synchronisation points read without a copy (h_obj + 1)
  volatile unsigned long long *h_status = nullptr;
  unsigned long long *d_hstatus = nullptr;
  // Asynchronous halo exchange (iem_halo_exchange_async): nothing is launched for it.  The exchange is DEFERRED and rides
  // on the first evaluation launch that takes the same x and cannot touch a halo entry of it: one extra leading workgroup
  // of that kernel (iem_halo_wg, through the kernel argument `comm` = d_comm) sends, receives and writes the halo entries
  // while the kernel's other workgroups evaluate; a launch that CAN touch a halo entry first gets the stand-alone
  // exchange kernel in front of it.  (A comm stream + events was measured: two cross-stream dependencies cost more —
  // ~8 us per step — than the 3-4 us stand-alone kernel they were meant to hide; tools/halo_overlap_probe.py.)
  bool halo_deferred = false;
  double *halo_vec = nullptr;
  void *d_comm = nullptr;        // IemHaloArgs in device memory (x unused: the carrier kernel passes its own)
  bool reads_halo_x[iem::KK_LAST + 1] = {}, reads_halo_v[iem::KK_LAST + 1] = {}, carrier[iem::KK_LAST + 1] = {};
  uint64_t nonce = 0;
  // chain KKT solver (iem_kkt_chain_*): one code object per (block size, border size)
  struct KktMod { unsigned elim_wg = 64; int elim_bpw = 1; hipModule_t mod = nullptr; hipFunction_t elim = nullptr, upd = nullptr, fwd = nullptr, bwd = nullptr, hub_z = nullptr, hub_widen = nullptr, hub_mask = nullptr, hub_ety = nullptr, hub_ex = nullptr, hub_leaf = nullptr, hub_diagmax = nullptr, fz = nullptr, fs = nullptr, bw = nullptr; int solve_bpw = 0;
                  // the multi-column solves (csrc/iem_kkt_many_device.h): many_r columns per chunk (KKT_MR of the module's source)
                  hipFunction_t fwd_m = nullptr, bwd_m = nullptr, fz_m = nullptr, fs_m = nullptr, bw_m = nullptr, move_m = nullptr, colsum_m = nullptr; int many_r = 1; };
  std::map<std::pair<int, int>, KktMod> kkt_mods;
  std::map<int, void *> d_arrays;  // model array id -> device copy
  std::vector<double> theta_host;
  bool jit = false;
  // The derived programs (kDerived), each over its own generator options, with its own source, cache key and buffers: generated
  // and loaded by the first call that needs it or by its prepare call — the model's program and its cache key do not know of them.
  LoadedProgram derived[D_COUNT];
  // `d_kkt_zero`: ncon zeros, the dual direction of an iem_kktprod call with d_v == NULL
  double *d_kkt_zero = nullptr;
  // `obj_factor`: what iem_obj_end multiplies the pending objective value with when `obj_scaled` (set by
  // iem_eval_trial_scaled, cleared by every arm)
  bool obj_scaled = false;
  double obj_factor = 1.0;
  // the hand-written code objects of kFixed, each loaded by the first call that needs it (fixed_object): `mod` set = loaded, every
  // kernel of its row resolved
  struct FixedObject { hipModule_t mod = nullptr; hipFunction_t fn[kFixedSlots] = {}; } fixed[F_COUNT];
  // the code object of the filter line search (iem_search_*): loaded by the first iem_search_create of the handle
  struct SearchObject { hipModule_t mod = nullptr; hipFunction_t begin = nullptr, trial = nullptr, accept = nullptr; } search;
  // the code object of the second-order correction (iem_soc_*): loaded by the first iem_soc_create of the handle
  struct SocObject { hipModule_t mod = nullptr; hipFunction_t open = nullptr, rhs = nullptr, trial = nullptr, accept = nullptr, select = nullptr; } soc;
  // the code object of the feasibility restoration phase (iem_resto_*): loaded by the first iem_resto_create of the handle
  struct RestoObject { hipModule_t mod = nullptr; hipFunction_t fn[12] = {}; } resto;
  FixedObject barrier_mu;      // the barrier kernels that read mu and tau from an iem_mu block (barrier_mu_source): loaded by the first bind
  struct MuObject { hipModule_t mod = nullptr; hipFunction_t error = nullptr, update = nullptr, reset = nullptr; } mu;
  struct AmuObject { hipModule_t mod = nullptr; hipFunction_t probe = nullptr, update = nullptr, reset = nullptr; } amu;      // the adaptive rule (iem_amu_*): loaded by the first iem_amu_create
  struct QfObject { hipModule_t mod = nullptr; hipFunction_t begin = nullptr, alpha = nullptr, value = nullptr, update = nullptr, reset = nullptr; } qf;      // the quality-function oracle (iem_qf_*): loaded by the first iem_qf_create
  struct MpcObject { hipModule_t mod = nullptr; hipFunction_t terms = nullptr, step = nullptr, select = nullptr, reset = nullptr; } mpc;      // Mehrotra's corrector (iem_mpc_*): loaded by the first iem_mpc_create
  struct InitObject { hipModule_t mod = nullptr; hipFunction_t ls_terms = nullptr, ls_norm = nullptr, ls_apply = nullptr, warm = nullptr, mu = nullptr, reset = nullptr; } init;      // the starting point (iem_init_*): loaded by the first iem_init_create
  struct ConvObject { hipModule_t mod = nullptr; hipFunction_t xmax = nullptr, decide = nullptr, stepmax = nullptr, step_decide = nullptr, keep = nullptr, restore = nullptr, reset = nullptr; } conv;      // the stopping test (iem_conv_*): loaded by the first iem_conv_create
  RestoObject resto_mu;      // the restoration kernels that read mu, tau and zeta from an iem_mu block (resto_mu_source): loaded by the first iem_resto_bind_mu
  struct RmuObject { hipModule_t mod = nullptr; hipFunction_t error = nullptr, enter = nullptr, update = nullptr, trigger = nullptr, gather = nullptr; } rmu;      // the restoration's barrier parameter (iem_rmu_*): loaded by the first iem_rmu_create
  // `kb_part`: the column sums' workspace of the raw calls iem_kkt_border_factor / _solve (grown on demand)
  double *kb_part = nullptr;
  int64_t kb_part_n = 0;
  // the explicit blocks in COO (iem_jacp_coord / iem_hessp_coord).  `pc_view`: the parameter view with the blocks' layout
  // (param_coord_layout), built by the first structure / nnz / evaluation call; it points into `model`.  `d_pc_spare`: where a
  // block the caller passed NULL for is written when it is not empty (allocated by the first such call)
  iem::Model pc_view;
  bool pc_have_view = false;
  double *d_pc_spare[2] = {nullptr, nullptr};
};

namespace {

int upload_array(iem_model *m, int id, bool as_int) {
  if (m->d_arrays.count(id)) return IEM_OK;
  const iem::ArrayDesc &a = m->model.arrs[id];
  void *d = nullptr;
  size_t bytes = (size_t)std::max<int64_t>(a.n, 1) * 8;
  HIP_TRY(hipMalloc(&d, bytes));
  if ((a.kind == IEM_A_F64_DATA && !as_int) || (a.kind == IEM_A_I64_DATA && as_int)) {   // stored as requested: as is
    HIP_TRY(hipMemcpy(d, a.data, (size_t)a.n * 8, hipMemcpyHostToDevice));
  } else {   // the other stored type, or a fill / range array: converted element by element
    std::vector<uint64_t> tmp((size_t)a.n);
    for (int64_t j = 0; j < a.n; ++j) {
      if (as_int) tmp[j] = (uint64_t)a.i(j);
      else { const double v = a.f(j); std::memcpy(&tmp[j], &v, 8); }
    }
    HIP_TRY(hipMemcpy(d, tmp.data(), (size_t)a.n * 8, hipMemcpyHostToDevice));
  }
  m->d_arrays[id] = d;
  return IEM_OK;
}

// hiprtc build of the model's kernels for the handle's device; stores the code object in the cache
int jit_compile(iem_model *m, const std::string &src, const std::string &dir, const std::string &path, std::vector<char> &code) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, m->device));
  std::string arch = prop.gcnArchName;
  size_t colon = arch.find(':');
  if (colon != std::string::npos) arch = arch.substr(0, colon);
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "iem_kernels.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    return fail(IEM_E_COMPILE, "hiprtcCreateProgram failed");
  std::string archopt = "--offload-arch=" + arch;
  std::string cflag = contract_flag(m->opt);
  if (src.rfind("// iem-flags:", 0) == 0) {      // the source's own flag line decides (the offline build reads the same line)
    const size_t eol = src.find('\n'), p = src.find("-ffp-contract=");
    if (p != std::string::npos && p < eol) cflag = src.substr(p, src.find_first_of(" \n", p) - p);
  }
  const char *opts[] = {archopt.c_str(), "-O3", cflag.c_str(), "-std=c++17"};
  hiprtcResult r = hiprtcCompileProgram(prog, 4, opts);
  if (r != HIPRTC_SUCCESS) {
    size_t n = 0;
    hiprtcGetProgramLogSize(prog, &n);
    std::string log(n, '\0');
    if (n) hiprtcGetProgramLog(prog, &log[0]);
    hiprtcDestroyProgram(&prog);
    return fail(IEM_E_COMPILE, "hiprtc: " + log);
  }
  size_t n = 0;
  hiprtcGetCodeSize(prog, &n);
  code.resize(n);
  hiprtcGetCode(prog, code.data());
  hiprtcDestroyProgram(&prog);
  m->jit = true;
  mkdir(dir.c_str(), 0755);
  // several ranks may compile the same key at once: private temp name, atomic rename
  const std::string tmp = path + ".tmp." + std::to_string((long long)getpid());
  std::ofstream f(tmp, std::ios::binary);
  if (f) {
    f.write(code.data(), (std::streamsize)code.size());
    f.close();
    if (std::rename(tmp.c_str(), path.c_str()) != 0) std::remove(tmp.c_str());
  }
  return IEM_OK;
}

// code object of a complete HIP source (code-object cache next to the library -> hiprtc on a miss)
int load_source(iem_model *m, const std::string &src, hipModule_t *mod) {
  const uint64_t key = iem::fnv1a64(src);
  const std::string dir = cache_dir();
  const std::string path = dir + "/iem_" + key_hex(key) + ".hsaco";
  std::vector<char> code;
  bool loaded = false;
  if (read_file(path, code)) {
    // a cached object that does not load (truncated file, built for another architecture) is rebuilt
    loaded = hipModuleLoadData(mod, code.data()) == hipSuccess;
    if (!loaded) { *mod = nullptr; (void)hipGetLastError(); }
  }
  if (!loaded) {
    int rc = jit_compile(m, src, dir, path, code);
    if (rc) return rc;
    HIP_TRY(hipModuleLoadData(mod, code.data()));
  }
  return IEM_OK;
}

// A hand-written code object: the module of `src` and the kernels its `n` slots name.  *mod and the slots' functions are written
// only once every name is resolved; any failure unloads the module and leaves them as they were (never loaded).
struct KernelSlot { const char *name; hipFunction_t *fn; };
int load_object(iem_model *m, const std::string &src, const KernelSlot *slots, int n, hipModule_t *mod) {
  hipModule_t loaded = nullptr;
  int rc = load_source(m, src, &loaded);
  if (rc) return rc;
  std::vector<hipFunction_t> fns((size_t)n);
  for (int i = 0; i < n; ++i) {
    const hipError_t e = hipModuleGetFunction(&fns[i], loaded, slots[i].name);
    if (e != hipSuccess) {
      hipModuleUnload(loaded);
      return fail(IEM_E_HIP, std::string("hipModuleGetFunction(") + slots[i].name + "): " + hipGetErrorString(e));
    }
  }
  for (int i = 0; i < n; ++i) *slots[i].fn = fns[i];
  *mod = loaded;
  return IEM_OK;
}

// row `f` of kFixed on the handle: loaded by the first call
int fixed_object(iem_model *m, Fixed f) {
  iem_model::FixedObject &o = m->fixed[f];
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = fixed_source(f, src);
  if (rc) return rc;
  KernelSlot slots[kFixedSlots];
  int n = 0;
  for (; n < kFixedSlots && kFixed[f].kernels[n]; ++n) slots[n] = KernelSlot{kFixed[f].kernels[n], &o.fn[n]};
  return load_object(m, src, slots, n, &o.mod);
}

// code object of `co.prog` (generated with `opt`) and its kernel functions
int load_program(iem_model *m, CodeObject &co, const iem::Options &opt) {
  int rc = load_source(m, full_source(co.prog, opt), &co.mod);
  if (rc) return rc;
  co.fns.resize(co.prog.kernels.size());
  for (size_t k = 0; k < co.prog.kernels.size(); ++k)
    HIP_TRY(hipModuleGetFunction(&co.fns[k], co.mod, co.prog.kernels[k].name.c_str()));
  return IEM_OK;
}

// frees whatever of `P` exists and leaves it as never set up
void release_program(LoadedProgram &P) {
  for (double *r : P.d_red) if (r) hipFree(r);
  for (long long *r : P.d_axis) if (r) hipFree(r);
  for (long long *r : P.d_gather) if (r) hipFree(r);
  if (P.d_partials) hipFree(P.d_partials);
  for (void *t : P.d_tables) if (t) hipFree(t);
  if (P.mod) hipModuleUnload(P.mod);
  P = LoadedProgram();
}

int compile_or_load(iem_model *m) {
  int rc = load_program(m, m->code, m->opt);
  if (rc) return rc;
  HIP_TRY(hipModuleGetFunction(&m->fn_struct, m->code.mod, "iem_structure_kernel"));
  HIP_TRY(hipModuleGetFunction(&m->fn_csr, m->code.mod, "iem_csr_gather_sum"));
  HIP_TRY(hipModuleGetFunction(&m->fn_csr32, m->code.mod, "iem_csr_gather_sum32"));
  HIP_TRY(hipModuleGetFunction(&m->fn_spmv, m->code.mod, "iem_csr_spmv_kernel"));
  HIP_TRY(hipModuleGetFunction(&m->fn_spmv_long, m->code.mod, "iem_csr_spmv_long_kernel"));
  HIP_TRY(hipModuleGetFunction(&m->fn_axis, m->code.mod, "iem_axis_sum_kernel"));
  HIP_TRY(hipModuleGetFunction(&m->fn_gather, m->code.mod, "iem_gather_sum_kernel"));
  HIP_TRY(hipModuleGetFunction(&m->fn_halo, m->code.mod, m->opt.two_sided ? "iem_halo2_kernel" : "iem_halo_kernel"));
  HIP_TRY(hipModuleGetFunction(&m->fn_fold, m->code.mod, m->opt.two_sided ? "iem_halo2_fold_kernel" : "iem_halo_fold_kernel"));
  HIP_TRY(hipModuleGetFunction(&m->fn_reduce, m->code.mod, "iem_allreduce_kernel"));
  return IEM_OK;
}

// One launch of a kernel that takes its arguments as ONE block of `sz` bytes (every hand-written kernel and every generated one does)
int launch_args(hipFunction_t fn, void *args, size_t sz, unsigned gx, unsigned gy, unsigned block, unsigned lds, hipStream_t stream, unsigned gz = 1) {
  void *cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(fn, gx, gy, gz, block, 1, 1, lds, stream, nullptr, cfg));
  return IEM_OK;
}

// The head of every generated kernel's argument block (iem_codegen.cpp: emit_kernel_head), the only part rewritten per
// launch.  The last five words carry the further outputs of the one-launch kinds (iem_codegen.hpp: KernelKind).
struct LaunchHead {
  const double *x = nullptr, *th = nullptr, *y = nullptr, *v = nullptr;
  double *out = nullptr;
  double w = 0.0;
  double *aux = nullptr;
  const void *comm = nullptr;   // set by launch_kind: the deferred halo exchange this launch carries (IemHaloArgs)
  union {
    double *g = nullptr;        // KK_ACCEPTED / KK_ALL: grad!'s output
    double *trial_partials;     // KK_TRIAL: the objective's partials
  };
  union {
    double *g_red = nullptr;    // KK_ACCEPTED / KK_ALL: grad!'s reduction buffer
    double *lag_out;            // KK_TRIAL of the residual program: lagrad's output
  };
  union {
    double *c = nullptr;        // KK_ALL: cons!'s output
    double *lag_red;            // KK_TRIAL of the residual program: lagrad's reduction buffer
  };
  double *partials = nullptr;   // KK_ALL: the objective's partials
  double *obj = nullptr;        // KK_ALL: the objective scalar
};
static_assert(sizeof(LaunchHead) == 13 * 8, "the generated Args_* head is 13 words");

// a kernel's tables {ip, dp, fa, ia} as words (an empty table still takes one): inline in its argument block, or in a
// device copy the block points to when they do not fit (KernelDesc::tables_in_memory)
void pack_tables(iem_model *m, const iem::KernelDesc &kd, std::vector<uint64_t> &out) {
  for (int64_t v : kd.ip) out.push_back((uint64_t)v);
  if (kd.ip.empty()) out.push_back(0);
  for (double v : kd.dp) { uint64_t b; std::memcpy(&b, &v, 8); out.push_back(b); }
  if (kd.dp.empty()) out.push_back(0);
  for (int id : kd.fa) out.push_back((uint64_t)(uintptr_t)m->d_arrays[id]);
  if (kd.fa.empty()) out.push_back(0);
  for (int id : kd.ia) out.push_back((uint64_t)(uintptr_t)m->d_arrays[id]);
  if (kd.ia.empty()) out.push_back(0);
}

// uploads what the program's kernels read and builds, once, their argument blocks and lists of launchable kernels
int prepare_program(iem_model *m, CodeObject &co) {
  int rc;
  for (const iem::KernelDesc &kd : co.prog.kernels) {
    for (int id : kd.fa) if ((rc = upload_array(m, id, false)) != IEM_OK) return rc;
    for (int id : kd.ia) if ((rc = upload_array(m, id, true)) != IEM_OK) return rc;
  }
  const size_t n = co.prog.kernels.size();
  co.d_tables.assign(n, nullptr);
  co.argbuf.resize(n);
  for (size_t k = 0; k < n; ++k) {
    const iem::KernelDesc &kd = co.prog.kernels[k];
    std::vector<uint64_t> &buf = co.argbuf[k];
    buf.assign(sizeof(LaunchHead) / 8, 0);
    if (kd.tables_in_memory) {
      std::vector<uint64_t> tb;
      pack_tables(m, kd, tb);
      HIP_TRY(hipMalloc(&co.d_tables[k], tb.size() * 8));
      HIP_TRY(hipMemcpy(co.d_tables[k], tb.data(), tb.size() * 8, hipMemcpyHostToDevice));
      const uint64_t *t = (const uint64_t *)co.d_tables[k];
      const size_t nip = std::max<size_t>(1, kd.ip.size()), ndp = std::max<size_t>(1, kd.dp.size()), nfa = std::max<size_t>(1, kd.fa.size());
      for (const uint64_t *p : {t, t + nip, t + nip + ndp, t + nip + ndp + nfa}) buf.push_back((uint64_t)(uintptr_t)p);
    } else {
      pack_tables(m, kd, buf);
    }
    if (kd.kind >= 0 && kd.kind <= iem::KK_LAST && kd.n_blocks > 0) co.launchable[kd.kind].push_back((int)k);   // (a grid none of whose templates has an item: nothing to launch)
  }
  return IEM_OK;
}

// A mailbox wait timed out since the last check: the kernels poisoned what they delivered (NaN) and recorded it in
// mapped host memory.  Host synchronisation points (iem_obj / iem_obj_end / iem_synchronize) report it once and clear it.
int comm_check(iem_model *m) {
  if (!m->h_status || *m->h_status == 0) return IEM_OK;
  const unsigned long long bits = *m->h_status;
  *m->h_status = 0;
  if (m->mailbox) { const unsigned long long z = 0; (void)hipMemcpy(m->mailbox, &z, 8, hipMemcpyHostToDevice); (void)hipGetLastError(); }
  return fail(IEM_E_COMM, "a mailbox wait timed out (status bits " + std::to_string(bits) + ": 1/2 halo ack/data, 4 all-reduce, 8/16 fold ack/data; 32/64 and 128/256: the same of the second direction): "
                          "a peer did not take part in the exchange; the halo entries / reduced values it should have delivered were set to NaN");
}

// the all-reduce runs on G workgroups, each on its own chunk of the NR doubles (one per 1 024, at most 64)
int64_t reduce_chunks(int64_t NR) { return std::min<int64_t>(64, std::max<int64_t>(1, (NR + 1023) / 1024)); }
// IemHaloArgs, and behind it what IemHalo2Args adds (iem_halo2_device.h); a one-way shard's kernels take the first 11 words only
struct HaloArgsH { double *x; unsigned long long *mine, *left, *right; const long long *src, *dst; long long NH, W, G; unsigned long long *hstatus; long long ticks;
                   const long long *src_l, *dst_r; long long NL, B2; };
constexpr size_t kHaloArgs1 = 11 * 8;
// word offset of the second direction's block in a mailbox: behind the fold data of the one-way layout
int64_t mailbox_b2(int64_t W, int64_t NH, int64_t NR) {
  const int64_t G = reduce_chunks(NR);
  return 12 + G + 2 * W * G + 2 * NH + 2 * W * NR + 2 * NH;
}
HaloArgsH halo_args(iem_model *m, double *d_x) {
  const iem::ShardInfo &si = m->shard;
  return HaloArgsH{d_x, m->mailbox, si.rank > 0 ? m->peers[si.rank - 1] : nullptr, si.rank + 1 < si.world ? m->peers[si.rank + 1] : nullptr,
                   m->d_halo_src, m->d_halo_dst, (long long)si.halo_doubles, (long long)si.world, (long long)reduce_chunks(1 + m->n_shared),
                   m->d_hstatus, (long long)m->opt.comm_timeout_ms * 100000LL,
                   m->d_halo_src_l, m->d_halo_dst_r, (long long)si.halo_doubles_right, (long long)mailbox_b2(si.world, si.halo_doubles, 1 + m->n_shared)};
}
int halo_launch(iem_model *m, double *d_x, hipStream_t stream) {
  HaloArgsH A = halo_args(m, d_x);
  return launch_args(m->fn_halo, &A, m->opt.two_sided ? sizeof A : kHaloArgs1, 1, 1, 256, 0, stream);
}
int halo_flush(iem_model *m) {
  if (!m->halo_deferred) return IEM_OK;
  m->halo_deferred = false;
  return halo_launch(m, m->halo_vec, m->stream);
}
// Ordering of an evaluation call against a DEFERRED halo exchange (iem_halo_exchange_async), decided for the call about to
// be launched: a kind that can touch a halo entry of the exchanged vector (through x, or through a variable-space v) gets
// the stand-alone exchange kernel in front of it; otherwise, if it takes the same x and is a carrier kind, its first kernel
// CARRIES the exchange (*carry: one extra leading workgroup); otherwise nothing happens and the exchange stays deferred.
int halo_plan(iem_model *m, int kind, const void *x, const void *v, bool *carry) {
  *carry = false;
  if (!m->halo_deferred) return IEM_OK;
  const bool touches = (x == m->halo_vec && m->reads_halo_x[kind]) || (v && v == m->halo_vec && m->reads_halo_v[kind]);
  if (touches) return halo_flush(m);
  if (x == m->halo_vec && m->carrier[kind] && m->d_comm) { *carry = true; m->halo_deferred = false; }
  return IEM_OK;
}

// what runs BEHIND the kernels of a scatter kind (also behind the one-launch phases that contain grad!)
int kind_followups(iem_model *m, const LoadedProgram &P, int kind, double *out, double *aux) {
  const iem::Program &prog = P.prog;
  if (!prog.axis[kind].empty()) {   // sums over a non-lane axis: the rows the kernels parked -> one write per entry (iem_axis_sum_kernel)
    int64_t n0 = 1;
    for (auto &a : prog.axis[kind]) n0 = std::max(n0, a.n0);
    void *args[] = {(void *)&out, (void *)&aux, (void *)&P.d_axis[kind]};
    HIP_TRY(hipModuleLaunchKernel(m->fn_axis, (unsigned)((n0 + 63) / 64), (unsigned)prog.axis[kind].size(), 1, 256, 1, 1, 0, m->stream, args, nullptr));   // 64 lanes x 4 row groups per workgroup
  }
  if (!prog.gather[kind].dest.empty()) {   // what would have been float atomics: parked addends summed per entry in plan order
    const iem::Program::Gather &G = prog.gather[kind];
    long long n = (long long)G.dest.size();
    const double *parked = aux + G.aux_off;
    const long long *dest = P.d_gather[kind], *seg = dest + n;
    const void *perm = seg + n + 1;
    int wide = G.park_doubles >= (1LL << 32) ? 1 : 0;
    void *args[] = {(void *)&out, (void *)&parked, (void *)&dest, (void *)&seg, (void *)&perm, (void *)&n, (void *)&wide};
    HIP_TRY(hipModuleLaunchKernel(m->fn_gather, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, m->stream, args, nullptr));
  }
  return IEM_OK;
}

// device buffers of a program's scatter kinds: the aux buffer (shared-entry values x workgroups + ticket words, zeroed once,
// then the rows of its axis sums and the parked addends), the plan of its gather, the table of its axis sums
// `on_stream`: zero the aux buffers on that stream (a program set up between launches of a running handle) instead of
// with a plain hipMemset (handle creation)
int scatter_buffers(LoadedProgram &P, const hipStream_t *on_stream = nullptr) {
  const iem::Program &prog = P.prog;
  for (int kind = 0; kind < iem::KK_COUNT; ++kind) {
    const size_t words = (size_t)prog.aux_doubles[kind];
    if (words == 0) continue;
    if (hipMalloc((void **)&P.d_red[kind], words * 8) != hipSuccess ||
        (on_stream ? hipMemsetAsync(P.d_red[kind], 0, words * 8, *on_stream) : hipMemset(P.d_red[kind], 0, words * 8)) != hipSuccess)
      return fail(IEM_E_HIP, "hipMalloc reduction buffer");
    if (!prog.gather[kind].dest.empty()) {
      const iem::Program::Gather &G = prog.gather[kind];
      const size_t nd = G.dest.size(), np = G.perm.size();
      const bool wide = G.park_doubles >= (1LL << 32);   // parked positions fit 32 bits otherwise: half the plan traffic
      std::vector<uint32_t> p32;
      if (!wide) { p32.resize(np); for (size_t k = 0; k < np; ++k) p32[k] = (uint32_t)G.perm[k]; }
      if (hipMalloc((void **)&P.d_gather[kind], (2 * nd + 1) * 8 + np * (wide ? 8 : 4)) != hipSuccess ||
          hipMemcpy(P.d_gather[kind], G.dest.data(), nd * 8, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(P.d_gather[kind] + nd, G.seg.data(), (nd + 1) * 8, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(P.d_gather[kind] + 2 * nd + 1, wide ? (const void *)G.perm.data() : (const void *)p32.data(), np * (wide ? 8 : 4), hipMemcpyHostToDevice) != hipSuccess)
        return fail(IEM_E_HIP, "hipMalloc gather plan");
    }
    if (!prog.axis[kind].empty()) {
      std::vector<long long> tab;
      for (auto &a : prog.axis[kind]) { tab.push_back(a.c); tab.push_back(a.k0); tab.push_back(a.n0); tab.push_back(a.rows); tab.push_back(a.off); }
      if (hipMalloc((void **)&P.d_axis[kind], tab.size() * 8) != hipSuccess ||
          hipMemcpy(P.d_axis[kind], tab.data(), tab.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
        return fail(IEM_E_HIP, "hipMalloc axis-sum table");
    }
  }
  return IEM_OK;
}

// the partials of the program's objective kernels + the ticket counters behind them (iem_block_partial: 1 top + one per 32
// workgroups), zeroed once — the workgroups that complete a count reset it.  `on_stream` as for scatter_buffers
int partials_buffer(LoadedProgram &P, const hipStream_t *on_stream = nullptr) {
  const size_t np = (size_t)std::max<int64_t>(P.prog.n_partials, 1);
  const size_t words = np + 1 + (np + 31) / 32;
  if (hipMalloc((void **)&P.d_partials, words * 8) != hipSuccess) { P.d_partials = nullptr; return fail(IEM_E_HIP, "hipMalloc partials"); }
  if (on_stream) {
    if (hipMemsetAsync(P.d_partials, 0, words * 8, *on_stream) != hipSuccess) return fail(IEM_E_HIP, "hipMemsetAsync partials");
  } else if (hipMemset(P.d_partials, 0, words * 8) != hipSuccess) {
    return fail(IEM_E_HIP, "hipMalloc partials");
  }
  return IEM_OK;
}

// kernel k of `co` with the head `h` (h.comm set: the launch carries the deferred halo exchange — one extra leading workgroup column, iem_halo_wg)
int launch_one(iem_model *m, CodeObject &co, int k, const LaunchHead &h) {
  const iem::KernelDesc &kd = co.prog.kernels[k];
  const bool carry = h.comm != nullptr;
  std::vector<uint64_t> &buf = co.argbuf[k];
  std::memcpy(buf.data(), &h, sizeof h);
  return launch_args(co.fns[k], buf.data(), buf.size() * 8, (unsigned)kd.grid[0] + (carry ? 1u : 0u), (unsigned)kd.grid[1], (unsigned)kd.block, 0, m->stream,
                     (unsigned)kd.grid[2]);
}

// One evaluation call: the launchable kernels of `kind` in `P` with the head `h` (th and comm filled in here), ordered
// against a deferred halo exchange (halo_plan) — the first kernel launched carries it, and it stays deferred when the kind
// launches nothing — then a scatter kind's own follow-ups.  What runs behind a phase kind (grad!'s follow-ups behind the
// phases that contain it, lagrad's and kktx's behind their programs' KK_TRIAL) is the caller's to launch.
int launch_kind(iem_model *m, LoadedProgram &P, int kind, const LaunchHead &h) {
  bool carry = false;
  int rc = halo_plan(m, kind, h.x, h.v, &carry);
  if (rc) return rc;
  LaunchHead a = h;
  a.th = m->d_theta;
  for (int k : P.launchable[kind]) {
    a.comm = carry ? m->d_comm : nullptr;
    if ((rc = launch_one(m, P, k, a))) return rc;
    carry = false;
  }
  if (carry) m->halo_deferred = true;
  return kind < iem::KK_COUNT ? kind_followups(m, P, kind, h.out, h.aux) : IEM_OK;
}

// memsets what the kernels of a scatter kind of `P` do not overwrite completely, in front of them
int zero_uncovered(iem_model *m, const LoadedProgram &P, int kind, double *out) {
  for (auto &z : P.zero_ranges[kind])
    HIP_TRY(hipMemsetAsync(out + z.first, 0, (size_t)(z.second - z.first) * 8, m->stream));
  return IEM_OK;
}

// a scatter kind as its own call: the memsets, the kernels with the kind's reduction buffer as aux, the follow-ups
int launch_scatter(iem_model *m, LoadedProgram &P, int kind, LaunchHead h) {
  int rc = zero_uncovered(m, P, kind, h.out);
  if (rc) return rc;
  h.aux = P.d_red[kind];
  return launch_kind(m, P, kind, h);
}

// the tuner's record of jac_coord! (which = 0) / hess_coord! (1) into the buffer `out`; a buffer not seen lately takes the oldest slot, undecided
iem_model::Tune &tune_slot(iem_model *m, int which, const void *out) {
  iem_model::TuneSet &S = m->tune[which];
  iem_model::Tune *hit = nullptr;
  for (auto &t : S.slot)
    if (t.out == out) hit = &t;
  if (!hit) {
    hit = &S.slot[S.next];
    S.next = (S.next + 1) % 4;
    hit->out = out; hit->calls = 0; hit->choice = -1;
  }
  return *hit;
}

// jac_coord! / hess_coord! through the tuner (iem_model::alt): the first IEM_TUNE_CALLS calls into an output buffer
// run ten with the default, then ten with the alt object, under events; then the faster variant (medians of the last
// eight of each block; alt only if > 2 % faster) is kept.
int launch_tuned(iem_model *m, int which, int kind, const LaunchHead &h) {
  if (!m->alt.mod) return launch_kind(m, m->code, kind, h);
  iem_model::Tune &T = tune_slot(m, which, h.out);
  if (T.choice >= 0) return launch_kind(m, T.choice ? m->alt : m->code, kind, h);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(m->stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
  if (cap != hipStreamCaptureStatusNone) return launch_kind(m, m->code, kind, h);   // no timing inside a graph capture
  if (T.calls < IEM_TUNE_CALLS) {
    if (!T.have_events) {
      for (auto &e : T.ev) for (auto &q : e) HIP_TRY(hipEventCreate(&q));
      T.have_events = true;
    }
    const int v = T.calls >= IEM_TUNE_CALLS / 2 ? 1 : 0;   // a block of each: alternating single launches measures the switch, not the variant
    HIP_TRY(hipEventRecord(T.ev[T.calls][0], m->stream));
    int rc = launch_kind(m, v ? m->alt : m->code, kind, h);
    HIP_TRY(hipEventRecord(T.ev[T.calls][1], m->stream));
    ++T.calls;
    return rc;
  }
  if (hipEventQuery(T.ev[IEM_TUNE_CALLS - 1][1]) == hipSuccess) {   // all have run: decide (never waits)
    // single launches time to +-5 % and the first ones of a process run cold: median of each variant's last
    // eight samples; the large batch must win by 2 %
    std::vector<float> s[2];
    for (int c = 0; c < IEM_TUNE_CALLS; ++c) {
      const int v = c >= IEM_TUNE_CALLS / 2 ? 1 : 0;
      if (c - v * (IEM_TUNE_CALLS / 2) < 2) continue;   // the first two launches of a block: cold instruction cache, the other variant's tail
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, T.ev[c][0], T.ev[c][1]) == hipSuccess) s[v].push_back(ms);
    }
    float med[2] = {0.f, 1e30f};
    for (int v = 0; v < 2; ++v)
      if (!s[v].empty()) { std::sort(s[v].begin(), s[v].end()); med[v] = s[v][s[v].size() / 2]; }
    T.choice = med[1] < 0.98f * med[0] ? 1 : 0;
    if (getenv("IEM_TUNER_LOG")) {
      fprintf(stderr, "iem tuner: kind %d buffer %p:", kind, (const void *)h.out);
      for (int c = 0; c < IEM_TUNE_CALLS; ++c) { float ms = -1.f; (void)hipEventElapsedTime(&ms, T.ev[c][0], T.ev[c][1]); fprintf(stderr, " %s%.4f", c >= IEM_TUNE_CALLS / 2 ? "a" : "d", ms); }
      fprintf(stderr, " medians %.4f / %.4f -> %s\n", med[0], med[1], T.choice ? "alt" : "default");
    }
    return launch_kind(m, T.choice ? m->alt : m->code, kind, h);
  }
  (void)hipGetLastError();
  return launch_kind(m, m->code, kind, h);
}

// host-side item index evaluation for the structure calls
struct ItemIdx {
  const iem::Model &m;
  const iem::Template &t;
  std::vector<int64_t> ifv, idx;
  ItemIdx(const iem::Model &mm, const iem::Template &tt) : m(mm), t(tt), ifv(tt.ifields.size()), idx(tt.idx.size()) {}
  void eval(int64_t k) {
    int64_t kc[3] = {k % t.dims[0], (k / t.dims[0]) % t.dims[1], k / (t.dims[0] * t.dims[1])};
    for (size_t f = 0; f < t.ifields.size(); ++f) {
      const iem::FieldDesc &fl = t.ifields[f];
      int64_t p = fl.base + fl.step[0] * kc[0] + fl.step[1] * kc[1] + fl.step[2] * kc[2];
      ifv[f] = fl.mode == IEM_F_AFFINE ? p : m.arrs[fl.arr].i(p);
    }
    for (size_t i = 0; i < t.idx.size(); ++i) {
      int64_t v = t.idx[i].c0;
      for (int j = 0; j < t.idx[i].nterms; ++j) v += t.idx[i].coef[j] * ifv[t.idx[i].field[j]];
      idx[i] = v;
    }
  }
};

// host mirrors of the device structs in iem_device.h
struct IdxDescH {
  long long c, k[3];
  int ng, garr[3];
  long long gcoef[3], gbase[3], gstep[3][3];
};
struct StructArgsH {
  long long *rows, *cols;
  const IdxDescH *ia, *ib;
  const long long *const *iarrs;
  long long dims0, dims1, n_items, o, o0, base;
  int nslots;
};

IdxDescH make_idx_desc(const iem::Template &t, int idx_id, const std::map<int, int> &iarr_slot) {
  IdxDescH d;
  std::memset(&d, 0, sizeof d);
  const iem::IdxExpr &ix = t.idx[idx_id];
  d.c = ix.c0;
  for (int j = 0; j < ix.nterms; ++j) {
    const iem::FieldDesc &f = t.ifields[ix.field[j]];
    if (f.mode == IEM_F_AFFINE) {
      d.c += ix.coef[j] * f.base;
      for (int dd = 0; dd < 3; ++dd) d.k[dd] += ix.coef[j] * f.step[dd];
    } else {
      int g = d.ng++;
      d.garr[g] = iarr_slot.at(f.arr);
      d.gcoef[g] = ix.coef[j];
      d.gbase[g] = f.base;
      for (int dd = 0; dd < 3; ++dd) d.gstep[g][dd] = f.step[dd];
    }
  }
  return d;
}

int structure_device(iem_model *m, int64_t *d_rows, int64_t *d_cols, int base, bool hess) {
  // int64 columns referenced by index expressions → device table
  std::map<int, int> slot;
  std::vector<const long long *> ptrs;
  for (const iem::Template &t : m->model.tpl)
    for (const iem::FieldDesc &f : t.ifields)
      if (f.mode == IEM_F_GATHER && !slot.count(f.arr)) {
        int rc = upload_array(m, f.arr, true);
        if (rc) return rc;
        slot[f.arr] = (int)ptrs.size();
        ptrs.push_back((const long long *)m->d_arrays[f.arr]);
      }
  // scratch descriptors live until the structure kernels have drained; freed on every exit path
  // (hipFree waits for the device)
  struct Scratch {
    std::vector<void *> v;
    void push_back(void *p) { v.push_back(p); }
    ~Scratch() { for (void *p : v) hipFree(p); }
  } to_free;
  const long long **d_ptrs = nullptr;
  HIP_TRY(hipMalloc((void **)&d_ptrs, std::max<size_t>(ptrs.size(), 1) * 8));
  to_free.push_back((void *)d_ptrs);
  if (!ptrs.empty()) HIP_TRY(hipMemcpy(d_ptrs, ptrs.data(), ptrs.size() * 8, hipMemcpyHostToDevice));
  int rc = IEM_OK;
  if (hess && !m->code.prog.hess_classes.empty()) {
    for (const iem::HessClass &hc : m->code.prog.hess_classes) {
      const int ns = (int)hc.idx_i.size();
      if (ns == 0) continue;
      std::vector<IdxDescH> a(ns), b(ns);
      for (int s = 0; s < ns; ++s) {
        a[s] = make_idx_desc(m->model.tpl[hc.idx_i[s] / 65536], hc.idx_i[s] % 65536, slot);
        b[s] = make_idx_desc(m->model.tpl[hc.idx_j[s] / 65536], hc.idx_j[s] % 65536, slot);
      }
      IdxDescH *da = nullptr, *db = nullptr;
      HIP_TRY(hipMalloc((void **)&da, sizeof(IdxDescH) * ns)); to_free.push_back(da);
      HIP_TRY(hipMalloc((void **)&db, sizeof(IdxDescH) * ns)); to_free.push_back(db);
      HIP_TRY(hipMemcpy(da, a.data(), sizeof(IdxDescH) * ns, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(db, b.data(), sizeof(IdxDescH) * ns, hipMemcpyHostToDevice));
      const iem::Template &t = m->model.tpl[hc.tpl];
      StructArgsH A{(long long *)d_rows, (long long *)d_cols, da, db, d_ptrs, t.dims[0], t.dims[1], hc.n_items, hc.o, 0, base, ns};
      size_t sz = sizeof A;
      void *cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &A, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
      long long total = hc.n_items * ns;
      if (total == 0) continue;   // template without items (e.g. difference rows of a one-support grid)
      hipError_t e = hipModuleLaunchKernel(m->fn_struct, (unsigned)((total + 255) / 256), 1, 1, 256, 1, 1, 0, m->stream, nullptr, cfg);
      if (e != hipSuccess) { rc = fail(IEM_E_HIP, std::string("structure kernel: ") + hipGetErrorString(e)); break; }
    }
  } else
  for (const iem::Template &t : m->model.tpl) {
    int ns = hess ? t.o2step : t.o1step;
    if (ns == 0 || (!hess && t.kind != IEM_T_CON)) continue;
    std::vector<IdxDescH> a(ns), b(ns);
    for (int s = 0; s < ns; ++s) {
      a[s] = make_idx_desc(t, hess ? t.slot2_i[s] : t.slot1_idx[s], slot);
      if (hess) b[s] = make_idx_desc(t, t.slot2_j[s], slot);
    }
    IdxDescH *da = nullptr, *db = nullptr;
    HIP_TRY(hipMalloc((void **)&da, sizeof(IdxDescH) * ns));
    to_free.push_back(da);
    HIP_TRY(hipMemcpy(da, a.data(), sizeof(IdxDescH) * ns, hipMemcpyHostToDevice));
    if (hess) {
      HIP_TRY(hipMalloc((void **)&db, sizeof(IdxDescH) * ns));
      to_free.push_back(db);
      HIP_TRY(hipMemcpy(db, b.data(), sizeof(IdxDescH) * ns, hipMemcpyHostToDevice));
    }
    StructArgsH A{(long long *)d_rows, (long long *)d_cols, da, db, d_ptrs, t.dims[0], t.dims[1], t.n_items,
                  hess ? t.o2 : t.o1, t.o0, base, ns};
    size_t sz = sizeof A;
    void *cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &A, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    long long total = t.n_items * ns;
    if (total == 0) continue;
    hipError_t e = hipModuleLaunchKernel(m->fn_struct, (unsigned)((total + 255) / 256), 1, 1, 256, 1, 1, 0, m->stream, nullptr, cfg);
    if (e != hipSuccess) { rc = fail(IEM_E_HIP, std::string("structure kernel: ") + hipGetErrorString(e)); break; }
  }
  hipError_t e = hipStreamSynchronize(m->stream);
  if (rc) return rc;
  if (e != hipSuccess) return fail(IEM_E_HIP, std::string("structure kernel: ") + hipGetErrorString(e));
  return IEM_OK;
}

void jac_structure_host(const iem::Model &m, int64_t *rows, int64_t *cols, int base) {
  for (const iem::Template &t : m.tpl) {
    if (t.kind != IEM_T_CON || t.o1step == 0) continue;
    ItemIdx it(m, t);
    for (int64_t k = 0; k < t.n_items; ++k) {
      it.eval(k);
      int64_t o = t.o1 + (int64_t)t.o1step * k;
      for (int s = 0; s < t.o1step; ++s) {
        rows[o + s] = t.o0 + k + base;
        cols[o + s] = it.idx[t.slot1_idx[s]] - 1 + base;
      }
    }
  }
}

void hess_structure_merged_host(const iem::Model &m, const std::vector<iem::HessClass> &classes, int64_t *rows,
                                int64_t *cols, int base) {
  for (const iem::HessClass &hc : classes) {
    std::map<int, ItemIdx> evals;
    for (size_t s = 0; s < hc.idx_i.size(); ++s)
      for (int v : {hc.idx_i[s], hc.idx_j[s]})
        if (!evals.count(v / 65536)) evals.emplace(v / 65536, ItemIdx(m, m.tpl[v / 65536]));
    const int ns = (int)hc.idx_i.size();
    for (int64_t k = 0; k < hc.n_items; ++k) {
      for (auto &kv : evals) kv.second.eval(k);
      for (int s = 0; s < ns; ++s) {
        int64_t a = evals.at(hc.idx_i[s] / 65536).idx[hc.idx_i[s] % 65536];
        int64_t b = evals.at(hc.idx_j[s] / 65536).idx[hc.idx_j[s] % 65536];
        rows[hc.o + (int64_t)ns * k + s] = (a >= b ? a : b) - 1 + base;
        cols[hc.o + (int64_t)ns * k + s] = (a >= b ? b : a) - 1 + base;
      }
    }
  }
}

void hess_structure_host(const iem::Model &m, int64_t *rows, int64_t *cols, int base) {
  for (const iem::Template &t : m.tpl) {
    if (t.o2step == 0) continue;
    ItemIdx it(m, t);
    for (int64_t k = 0; k < t.n_items; ++k) {
      it.eval(k);
      int64_t o = t.o2 + (int64_t)t.o2step * k;
      for (int s = 0; s < t.o2step; ++s) {
        int64_t a = it.idx[t.slot2_i[s]], b = it.idx[t.slot2_j[s]];
        rows[o + s] = (a >= b ? a : b) - 1 + base;
        cols[o + s] = (a >= b ? b : a) - 1 + base;
      }
    }
  }
}

// the explicit θ blocks on a parameter view with its layout (iem_model.hpp: param_coord_layout); which: 0 dc/dθ (row = the
// constraint, column = the entry of θ), 1 d2L/dx dθ (row = the entry of x, column = the entry of θ, whichever operand
// order the slot has), 2 d2L/dθ2 (the triangle hess_structure_host reports: row >= column)
void param_coord_structure_host(const iem::Model &v, int which, int64_t *rows, int64_t *cols, int base) {
  for (const iem::Template &t : v.tpl) {
    const std::vector<int> &keep = which == 0 ? t.pc1 : which == 1 ? t.pcx : t.pcp;
    if (keep.empty()) continue;
    const int64_t o0 = which == 0 ? t.pc_o1 : which == 1 ? t.pc_ox : t.pc_op, ns = (int64_t)keep.size();
    ItemIdx it(v, t);
    for (int64_t k = 0; k < t.n_items; ++k) {
      it.eval(k);
      for (int64_t j = 0; j < ns; ++j) {
        const int s = keep[(size_t)j];
        const int64_t o = o0 + ns * k + j;
        if (which == 0) {
          rows[o] = t.o0 + k + base;
          cols[o] = it.idx[t.slot1_idx[s]] - 1 + base;
          continue;
        }
        const int64_t a = it.idx[t.slot2_i[s]], b = it.idx[t.slot2_j[s]];
        if (which == 1) {
          const bool a_theta = t.is_theta_idx(t.slot2_i[s]);
          rows[o] = (a_theta ? b : a) - 1 + base;
          cols[o] = (a_theta ? a : b) - 1 + base;
        } else {
          rows[o] = (a >= b ? a : b) - 1 + base;
          cols[o] = (a >= b ? b : a) - 1 + base;
        }
      }
    }
  }
}

}  // namespace

extern "C" {
static int create_impl(const void *blob, size_t nbytes, int device, const iem_option_t *opts, int n_opts, int shard_group,
                       int rank, int world, iem_model **out);


const char *iem_last_error(void) { return g_err.c_str(); }
const char *iem_version(void) { return "iem-hip 0.1 (gfx950)"; }

void iem_free(void *p) { std::free(p); }

static int apply_option(iem::Options &o, int &poll_obj, const char *name, int64_t value) {
  if (!name) return fail(IEM_E_ARG, "null option name");
  if (std::strcmp(name, "store_mode") == 0) { o.store_mode = (int)value; return IEM_OK; }
  if (std::strcmp(name, "nt_stores") == 0) { o.nt_stores = (int)value; return IEM_OK; }
  if (std::strcmp(name, "no_fuse") == 0) { o.no_fuse = (int)value; return IEM_OK; }
  if (std::strcmp(name, "poll_obj") == 0) { poll_obj = (int)value; return IEM_OK; }
  if (std::strcmp(name, "wide_stores") == 0) { o.wide_stores = (int)value; return IEM_OK; }
  if (std::strcmp(name, "overlap") == 0) { o.overlap = (int)value; return IEM_OK; }
  if (std::strcmp(name, "xcd_remap") == 0) { o.xcd_remap = (int)value; return IEM_OK; }
  if (std::strcmp(name, "split_small") == 0) { o.split_small = (int)value; return IEM_OK; }
  if (std::strcmp(name, "fuse_groups") == 0) { o.fuse_groups = (int)value; return IEM_OK; }
  if (std::strcmp(name, "fuse_zero") == 0) { o.fuse_zero = (int)value; return IEM_OK; }
  if (std::strcmp(name, "hess_merge") == 0) { o.hess_merge = (int)value; return IEM_OK; }
  if (std::strcmp(name, "ablate") == 0) { o.ablate = (int)value; return IEM_OK; }
  if (std::strcmp(name, "block") == 0) {
    if (value != 0 && (value < 64 || value > 1024 || value % 64)) return fail(IEM_E_ARG, "block must be 0 (chosen per model) or a multiple of 64 in 64..1024");
    o.block = (int)value;
    return IEM_OK;
  }
  if (std::strcmp(name, "lds_slots") == 0) { o.lds_slots = (int)value; return IEM_OK; }
  if (std::strcmp(name, "reorder") == 0) { o.reorder = (int)value; return IEM_OK; }
  if (std::strcmp(name, "min_waves") == 0) { o.min_waves = (int)value; return IEM_OK; }
  if (std::strcmp(name, "fp_contract") == 0) { o.fp_contract = (int)value; return IEM_OK; }
  if (std::strcmp(name, "obj_wgs") == 0) {
    if (value < 1 || value > 65536) return fail(IEM_E_ARG, "obj_wgs must be in 1..65536");
    o.obj_wgs = (int)value;
    return IEM_OK;
  }
  if (std::strcmp(name, "det_shared") == 0) { o.det_shared = (int)value; return IEM_OK; }
  if (std::strcmp(name, "flat2d") == 0) { o.flat2d = (int)value; return IEM_OK; }
  if (std::strcmp(name, "flush32") == 0) { o.flush32 = (int)value; return IEM_OK; }
  if (std::strcmp(name, "autotune") == 0) { o.autotune = (int)value; return IEM_OK; }
  if (std::strcmp(name, "pull_scatter") == 0) { o.pull_scatter = (int)value; return IEM_OK; }
  if (std::strcmp(name, "fold_colloc") == 0) { if (value < 0 || value > 2) return IEM_E_ARG; o.fold_colloc = (int)value; return IEM_OK; }
  if (std::strcmp(name, "fold_max_n") == 0) { if (value < 2 || value > 16) return IEM_E_ARG; o.fold_max_n = (int)value; return IEM_OK; }
  if (std::strcmp(name, "det_axis") == 0) { o.det_axis = (int)value; return IEM_OK; }
  if (std::strcmp(name, "det_scatter") == 0) { o.det_scatter = (int)value; return IEM_OK; }
  if (std::strcmp(name, "det_scatter_max") == 0) { o.det_scatter_max = value; return IEM_OK; }
  if (std::strcmp(name, "lazy_loads") == 0) { o.lazy_loads = (int)value; return IEM_OK; }
  if (std::strcmp(name, "lazy_min_loads") == 0) { o.lazy_min_loads = (int)value; return IEM_OK; }
  if (std::strcmp(name, "name_tag") == 0) { o.name_tag = (int)value; return IEM_OK; }
  if (std::strcmp(name, "lazy_all_kinds") == 0) { o.lazy_all_kinds = (int)value; return IEM_OK; }
  if (std::strcmp(name, "autotune_min_blocks") == 0) { o.autotune_min_blocks = (int)value; return IEM_OK; }
  if (std::strcmp(name, "big_batch_slots") == 0) { o.big_batch_slots = (int)value; return IEM_OK; }
  if (std::strcmp(name, "big_batch_jac") == 0) { o.big_batch_jac = value; return IEM_OK; }
  if (std::strcmp(name, "big_batch_hess") == 0) { o.big_batch_hess = value; return IEM_OK; }
  if (std::strcmp(name, "big_xcd") == 0) { o.big_xcd = (int)value; return IEM_OK; }
  if (std::strcmp(name, "big_tile") == 0) {
    if (value != 0 && (value < 64 || value > 1024 || value % 64)) return fail(IEM_E_ARG, "big_tile must be 0 (keep the model's tile) or a multiple of 64 in 64..1024");
    o.big_tile = (int)value;
    return IEM_OK;
  }
  if (std::strcmp(name, "pair_kernel") == 0) { o.pair_kernel = (int)value; return IEM_OK; }
  if (std::strcmp(name, "store_wait") == 0) { o.store_wait = (int)value; return IEM_OK; }
  if (std::strcmp(name, "carrier") == 0) { o.carrier = value != 0; return IEM_OK; }
  if (std::strcmp(name, "two_sided") == 0) { o.two_sided = value != 0; return IEM_OK; }
  if (std::strcmp(name, "phase_kernels") == 0) { o.phase_kernels = value != 0; return IEM_OK; }
  if (std::strcmp(name, "jac_split") == 0) { if (value < 0 || value > 1) return fail(IEM_E_ARG, "jac_split must be 0 or 1"); o.jac_split = (int)value; return IEM_OK; }
  if (std::strcmp(name, "cons_direct_2d") == 0) { o.cons_direct_2d = value != 0; return IEM_OK; }
  if (std::strcmp(name, "digit_fields") == 0) { o.digit_fields = value != 0; return IEM_OK; }
  if (std::strcmp(name, "param_kinds") == 0) { o.param_kinds = value >= 2 && value <= 5 ? (int)value : value != 0; return IEM_OK; }
  if (std::strcmp(name, "scaled_kinds") == 0) { if (value < 0 || value > 1) return fail(IEM_E_ARG, "scaled_kinds must be 0 or 1"); o.scaled_kinds = (int)value; return IEM_OK; }
  if (std::strcmp(name, "kkt_kinds") == 0) { if (value < 0 || value > 1) return fail(IEM_E_ARG, "kkt_kinds must be 0 or 1"); o.kkt_kinds = (int)value; return IEM_OK; }
  if (std::strcmp(name, "scaled_phase_kinds") == 0) { if (value < 0 || value > 1) return fail(IEM_E_ARG, "scaled_phase_kinds must be 0 or 1"); o.scaled_phase_kinds = (int)value; return IEM_OK; }
  if (std::strcmp(name, "comm_timeout_ms") == 0) {
    if (value < 1 || value > 600000) return fail(IEM_E_ARG, "comm_timeout_ms must be in 1..600000");
    o.comm_timeout_ms = (int)value;
    return IEM_OK;
  }
  return fail(IEM_E_ARG, std::string("unknown option ") + name);
}

int iem_set_option(const char *name, int64_t value) { return apply_option(g_opt, g_opt_poll_obj, name, value); }

int iem_emit_source(const void *blob, size_t nbytes, char **out_src, uint64_t *out_key) {
  try {
    iem::Model model;
    iem::parse_blob(blob, nbytes, model);
    iem::Program p = iem::generate(model, g_opt);
    return emit_out(full_source(p, g_opt), out_src, out_key);
  } catch (const std::exception &e) {
    return fail(IEM_E_BLOB, e.what());
  }
}

int iem_fixed_source(int index, const char **out_name, char **out_src, uint64_t *out_key) {
  if (index < 0 || index >= F_COUNT) return fail(IEM_E_ARG, "iem_fixed_source: no such code object");
  const int rc = fixed_source_out((Fixed)index, out_src, out_key);
  if (rc == IEM_OK && out_name) *out_name = kFixed[index].name;
  return rc;
}

int iem_emit_launch_plan(const void *blob, size_t nbytes, char **out_txt) {
  try {
    iem::Model model;
    iem::parse_blob(blob, nbytes, model);
    iem::Program p = iem::generate(model, g_opt);
    std::ostringstream os;
    os.precision(17);
    os << "partials " << p.n_partials << "\n";
    for (int kind = 0; kind < iem::KK_COUNT; ++kind)   // shared-entry reduction buffer of a scatter kind: values x workgroups (+ tickets)
      if (p.red_values[kind] > 0) os << "reduce " << kind << " " << p.red_values[kind] << " " << p.red_wgs[kind] << "\n";
    for (int kind = 0; kind < iem::KK_COUNT; ++kind) {   // whole aux buffer of a scatter kind, and its axis sums {c, k0, n0, rows, off}
      if (p.aux_doubles[kind] > 0) os << "aux " << kind << " " << p.aux_doubles[kind] << "\n";
      for (auto &a : p.axis[kind]) os << "axis " << kind << " " << a.c << " " << a.k0 << " " << a.n0 << " " << a.rows << " " << a.off << "\n";
      const iem::Program::Gather &G = p.gather[kind];
      if (!G.dest.empty()) {   // plan-driven gather: header, then the three arrays
        os << "gather " << kind << " " << G.aux_off << " " << G.park_doubles << " " << G.dest.size() << " " << G.perm.size() << "\n";
        os << "gdest"; for (int64_t v : G.dest) os << " " << v; os << "\n";
        os << "gseg"; for (int64_t v : G.seg) os << " " << v; os << "\n";
        os << "gperm"; for (int64_t v : G.perm) os << " " << v; os << "\n";
      }
    }
    for (int kind = 0; kind < iem::KK_COUNT; ++kind)   // ranges the runtime memsets before launching a scatter kind
      for (auto &z : p.zero_ranges[kind]) os << "zero " << kind << " " << z.first << " " << z.second << "\n";
    for (const iem::KernelDesc &kd : p.kernels) {
      os << "kernel " << kd.name << " kind " << kd.kind << " grid " << kd.grid[0] << " " << kd.grid[1] << " " << kd.grid[2]
         << " lds " << kd.lds_bytes << " rbytes " << kd.alg_bytes_read << " wbytes " << kd.alg_bytes_written << " block " << kd.block << " tim " << (kd.tables_in_memory ? 1 : 0) << "\n";
      os << "ip " << kd.ip.size(); for (int64_t v : kd.ip) os << " " << v; os << "\n";
      os << "dp " << kd.dp.size(); for (double v : kd.dp) { uint64_t b; std::memcpy(&b, &v, 8); os << " " << b; } os << "\n";
      os << "fa " << kd.fa.size(); for (int v : kd.fa) os << " " << v; os << "\n";
      os << "ia " << kd.ia.size(); for (int v : kd.ia) os << " " << v; os << "\n";
    }
    std::string s = os.str();
    if (out_txt) {
      *out_txt = (char *)std::malloc(s.size() + 1);
      std::memcpy(*out_txt, s.c_str(), s.size() + 1);
    }
    return IEM_OK;
  } catch (const std::exception &e) {
    return fail(IEM_E_BLOB, e.what());
  }
}

int iem_blob_array(const void *blob, size_t nbytes, int id, double **out_vals, int64_t *out_n) {
  if (!out_vals || !out_n) return fail(IEM_E_ARG, "null argument");
  try {
    iem::Model model;
    iem::parse_blob(blob, nbytes, model);
    if (id < 0 || id >= (int)model.arrs.size()) return fail(IEM_E_ARG, "array id out of range");
    const iem::ArrayDesc &a = model.arrs[id];
    double *v = (double *)std::malloc(sizeof(double) * (size_t)std::max<int64_t>(a.n, 1));
    for (int64_t j = 0; j < a.n; ++j) v[j] = a.f(j);
    *out_vals = v; *out_n = a.n;
    return IEM_OK;
  } catch (const std::exception &e) {
    return fail(IEM_E_BLOB, e.what());
  }
}

int iem_blob_hess_structure(const void *blob, size_t nbytes, int base, int64_t **out_rows, int64_t **out_cols, int64_t *out_nnz) {
  try {
    iem::Model model;
    iem::parse_blob(blob, nbytes, model);
    iem::Program p = iem::generate(model, g_opt);
    int64_t n = p.hess_classes.empty() ? model.nnzh : p.nnzh_merged;
    int64_t *r = (int64_t *)std::malloc(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1));
    int64_t *c = (int64_t *)std::malloc(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1));
    if (!p.hess_classes.empty()) hess_structure_merged_host(model, p.hess_classes, r, c, base);
    else hess_structure_host(model, r, c, base);
    *out_rows = r; *out_cols = c; *out_nnz = n;
    return IEM_OK;
  } catch (const std::exception &e) {
    return fail(IEM_E_BLOB, e.what());
  }
}

/* structure of one explicit θ block from a blob alone (no device): which = 0 dc/dθ, 1 d2L/dx dθ, 2 d2L/dθ2 */
int iem_blob_param_coord_structure(const void *blob, size_t nbytes, int which, int base, int64_t **out_rows, int64_t **out_cols, int64_t *out_nnz) {
  if (!out_rows || !out_cols || !out_nnz || which < 0 || which > 2) return fail(IEM_E_ARG, "bad argument");
  try {
    iem::Model model;
    iem::parse_blob(blob, nbytes, model);
    iem::Model view = iem::parameter_view(model);
    iem::param_coord_layout(view);
    const int64_t n = which == 0 ? view.nnzjp : which == 1 ? view.nnzhxp : view.nnzhpp;
    int64_t *r = (int64_t *)std::malloc(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1));
    int64_t *c = (int64_t *)std::malloc(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1));
    param_coord_structure_host(view, which, r, c, base);
    *out_rows = r; *out_cols = c; *out_nnz = n;
    return IEM_OK;
  } catch (const std::exception &e) {
    return fail(IEM_E_BLOB, e.what());
  }
}

int iem_create(const void *blob, size_t nbytes, int device, iem_model **out) {
  return iem_create_opts(blob, nbytes, device, nullptr, 0, out);
}

int iem_create_opts(const void *blob, size_t nbytes, int device, const iem_option_t *opts, int n_opts, iem_model **out) {
  return create_impl(blob, nbytes, device, opts, n_opts, 0, 0, 1, out);
}

int iem_create_sharded(const void *blob, size_t nbytes, int device, int group, int rank, int world,
                       const iem_option_t *opts, int n_opts, iem_model **out) {
  if (group < 1) return fail(IEM_E_ARG, "iem_create_sharded: group must be >= 1");
  return create_impl(blob, nbytes, device, opts, n_opts, group, rank, world, out);
}

static int create_impl(const void *blob, size_t nbytes, int device, const iem_option_t *opts, int n_opts, int shard_group,
                       int rank, int world, iem_model **out) {
  if (!blob || !out || n_opts < 0 || (n_opts && !opts)) return fail(IEM_E_ARG, "null argument");
  *out = nullptr;
  // the handle's options: the process defaults (iem_set_option) with this call's overrides on top
  iem::Options hopt = g_opt;
  int hpoll = g_opt_poll_obj;
  for (int i = 0; i < n_opts; ++i) {
    int rc = apply_option(hopt, hpoll, opts[i].name, opts[i].value);
    if (rc) return rc;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(IEM_E_NODEVICE, "no HIP device visible: libiem_hip has no CPU path");
  if (device < 0 || device >= ndev) return fail(IEM_E_ARG, "device ordinal out of range");
  iem_model *m = new iem_model();
  m->device = device;
  iem::select_program(hopt, iem::PG_MODEL);   // (the handle's own program; a derived program is selected by its row in kDerived)
  m->opt = hopt;
  m->poll_obj = hpoll;
  try {
    iem::parse_blob(blob, nbytes, m->model);
    if (shard_group > 0) {   // cut this rank's window out of the global model (iem_shard.hpp)
      iem::shard_model(m->model, shard_group, rank, world, m->shard);
      m->sharded = true;
      m->opt.carrier = 1;    // only a sharded handle's kernels carry the halo-exchange prologue (iem_halo_exchange_async)
      m->opt.two_sided = m->shard.reach_right > 0 ? 1 : 0;   // a stencil reaches to the right: the two-way exchange kernels join the source
      // continue from the shard's own blob — byte for byte what iem_shard_blob hands out — so that the
      // generated source (hence the code-object cache key) is the one an offline build of that blob gets,
      // and the global arrays nothing references any more (x0/lvar/uvar of the whole model) are released
      std::vector<int64_t> local = iem::serialize_model(m->model);
      m->model = iem::Model();
      iem::parse_blob(local.data(), local.size() * 8, m->model);
    }
    m->code.prog = iem::generate(m->model, m->opt);
  } catch (const std::exception &e) {
    delete m;
    return fail(IEM_E_BLOB, e.what());
  }
  int rc = IEM_OK;
  auto bail = [&](int code) { iem_destroy(m); return code; };
  if (hipSetDevice(device) != hipSuccess) return bail(fail(IEM_E_HIP, "hipSetDevice failed"));
  if ((rc = compile_or_load(m)) != IEM_OK) return bail(rc);
  const iem::Model &M = m->model;
  m->theta_host.resize((size_t)std::max<int64_t>(M.npar, 1));
  for (int64_t i = 0; i < M.npar; ++i) m->theta_host[i] = M.arrs[M.arr_theta].f(i);
  if (hipMalloc((void **)&m->d_theta, m->theta_host.size() * 8) != hipSuccess) return bail(fail(IEM_E_HIP, "hipMalloc theta"));
  if (hipMemcpy(m->d_theta, m->theta_host.data(), m->theta_host.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail(IEM_E_HIP, "upload theta"));
  if ((rc = partials_buffer(m->code)) != IEM_OK || (rc = scatter_buffers(m->code)) != IEM_OK) return bail(rc);
  if (hipHostMalloc((void **)&m->h_obj, 16, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void **)&m->d_hobj, m->h_obj, 0) != hipSuccess) return bail(fail(IEM_E_HIP, "hipHostMalloc"));
  m->h_status = reinterpret_cast<volatile unsigned long long *>(m->h_obj + 1);   // second word: comm time-outs (IemCommErr::hstatus)
  m->d_hstatus = reinterpret_cast<unsigned long long *>(m->d_hobj + 1);
  *m->h_status = 0;
  if (m->sharded) {
    // which kinds can touch a halo entry of x / of a variable-space v: from the live loads of the generated kernels
    const auto &flag = m->shard.var_flag;
    std::vector<int64_t> pre(flag.size() + 1, 0);
    for (size_t i = 0; i < flag.size(); ++i) pre[i + 1] = pre[i] + ((flag[i] & 12) ? 1 : 0);   // front and back halo copies alike
    auto hits = [&](const std::vector<std::pair<int64_t, int64_t>> &rs) {
      for (auto &r : rs) {
        const int64_t lo = std::max<int64_t>(0, r.first), hi = std::min<int64_t>((int64_t)flag.size() - 1, r.second);
        if (lo <= hi && pre[(size_t)hi + 1] - pre[(size_t)lo] > 0) return true;
      }
      return false;
    };
    for (const iem::KernelDesc &kd : m->code.prog.kernels) {
      if (kd.kind < 0 || kd.kind > iem::KK_LAST) continue;
      m->reads_halo_x[kd.kind] = m->reads_halo_x[kd.kind] || hits(kd.x_ranges);
      m->reads_halo_v[kd.kind] = m->reads_halo_v[kd.kind] || hits(kd.v_ranges);
    }
    // a kind can carry a deferred exchange when EVERY kernel of it has the carrier prologue (a phase kernel whose grad! member
    // reduces shared entries has none: one extra workgroup there would shift every tile)
    bool any[iem::KK_LAST + 1] = {}, all[iem::KK_LAST + 1];
    for (bool &a : all) a = true;
    for (const iem::KernelDesc &kd : m->code.prog.kernels) {
      if (kd.kind < 0 || kd.kind > iem::KK_LAST) continue;
      any[kd.kind] = true; all[kd.kind] = all[kd.kind] && kd.carries;
    }
    for (int k = 0; k <= iem::KK_LAST; ++k) m->carrier[k] = any[k] && all[k];
  }
  if ((rc = prepare_program(m, m->code)) != IEM_OK) return bail(rc);
  // second code object for the tuner: only for block-store models with a large jac/hess grid (below ~2e5 supports
  // the larger batch loses), never for the experiment knobs
  if (m->opt.autotune && m->opt.store_mode == 2 && m->opt.lds_slots < 48 && !m->opt.no_fuse && !m->opt.ablate) {
    int64_t big = 0;
    for (const iem::KernelDesc &kd : m->code.prog.kernels)
      if (kd.kind == iem::KK_JAC || kd.kind == iem::KK_HESS) big = std::max(big, kd.n_blocks);
    if (big >= m->opt.autotune_min_blocks) {
      iem::Options ob = m->opt;
      ob.lds_slots = 48;
      ob.name_tag = 48;
      try {
        m->alt.prog = iem::generate(m->model, ob);
      } catch (const std::exception &e) {
        return bail(fail(IEM_E_BLOB, e.what()));
      }
      if ((rc = load_program(m, m->alt, ob)) != IEM_OK || (rc = prepare_program(m, m->alt)) != IEM_OK) return bail(rc);
    }
  }
  for (int kind : {(int)iem::KK_GRAD, (int)iem::KK_JTPROD, (int)iem::KK_HPROD}) {
    // ranges the kernels of the kind do not overwrite completely.  Neighbouring ranges separated by a SHORT
    // fully-overwritten stretch are zeroed as one (what lies between is written afterwards, on the same
    // stream): one memset launch instead of two around pandemic's u(t) slab (grad! 11.5 -> 6 us of memsets)
    auto &zr = m->code.zero_ranges[kind];
    for (auto &z : m->code.prog.zero_ranges[kind]) {
      // the gap is measured against the two NEIGHBOURING ranges (never the whole span so far) and capped: a memset
      // never swallows more than 64 K doubles that a kernel is about to overwrite anyway
      const int64_t near = zr.empty() ? 0 : std::min<int64_t>(65536, std::max<int64_t>(8192, ((zr.back().second - zr.back().first) + (z.second - z.first)) / 16));
      if (!zr.empty() && z.first - zr.back().second <= near) zr.back().second = z.second;
      else zr.push_back(z);
    }
  }
  *out = m;
  return IEM_OK;
}

int iem_destroy(iem_model *m) {
  if (!m) return IEM_OK;
  DevGuard dg_(m->device);
  if (m->d_theta) hipFree(m->d_theta);
  for (void *p : m->ipc_opened) hipIpcCloseMemHandle(p);
  if (m->mailbox) hipFree(m->mailbox);
  if (m->d_peers) hipFree(m->d_peers);
  if (m->d_halo_src) hipFree(m->d_halo_src);
  if (m->d_halo_dst) hipFree(m->d_halo_dst);
  if (m->d_halo_src_l) hipFree(m->d_halo_src_l);
  if (m->d_halo_dst_r) hipFree(m->d_halo_dst_r);
  if (m->d_shared) hipFree(m->d_shared);
  if (m->h_obj) hipHostFree(m->h_obj);
  if (m->d_comm) hipFree(m->d_comm);
  for (auto &kv : m->kkt_mods) if (kv.second.mod) hipModuleUnload(kv.second.mod);
  for (auto &kv : m->d_arrays) hipFree(kv.second);
  release_program(m->alt);
  for (LoadedProgram &P : m->derived) release_program(P);
  if (m->d_kkt_zero) hipFree(m->d_kkt_zero);
  for (auto &o : m->fixed) if (o.mod) hipModuleUnload(o.mod);
  if (m->search.mod) hipModuleUnload(m->search.mod);
  if (m->soc.mod) hipModuleUnload(m->soc.mod);
  if (m->resto.mod) hipModuleUnload(m->resto.mod);
  if (m->mu.mod) hipModuleUnload(m->mu.mod);
  if (m->amu.mod) hipModuleUnload(m->amu.mod);
  if (m->qf.mod) hipModuleUnload(m->qf.mod);
  if (m->mpc.mod) hipModuleUnload(m->mpc.mod);
  if (m->init.mod) hipModuleUnload(m->init.mod);
  if (m->conv.mod) hipModuleUnload(m->conv.mod);
  if (m->resto_mu.mod) hipModuleUnload(m->resto_mu.mod);
  if (m->rmu.mod) hipModuleUnload(m->rmu.mod);
  if (m->barrier_mu.mod) hipModuleUnload(m->barrier_mu.mod);
  if (m->kb_part) hipFree(m->kb_part);
  for (double *r : m->d_pc_spare) if (r) hipFree(r);
  for (auto &S : m->tune) for (auto &T : S.slot) if (T.have_events) for (auto &e : T.ev) for (auto &q : e) hipEventDestroy(q);
  release_program(m->code);
  delete m;
  return IEM_OK;
}

int iem_meta(const iem_model *m, iem_meta_t *out) {
  if (!m || !out) return fail(IEM_E_ARG, "null argument");
  out->nvar = m->model.nvar; out->ncon = m->model.ncon; out->npar = m->model.npar;
  out->nnzj = m->model.nnzj;
  out->nnzh = m->code.prog.hess_classes.empty() ? m->model.nnzh : m->code.prog.nnzh_merged;
  out->n_templates = (int64_t)m->model.tpl.size();
  out->minimize = m->model.minimize;
  out->n_kernels = (int32_t)m->code.prog.kernels.size();
  return IEM_OK;
}

int iem_template_info(const iem_model *m, int64_t i, iem_template_info_t *out) {
  if (!m || !out || i < 0 || i >= (int64_t)m->model.tpl.size()) return fail(IEM_E_ARG, "bad template index");
  const iem::Template &t = m->model.tpl[i];
  out->kind = t.kind; out->n_items = t.n_items; out->o0 = t.o0; out->o1 = t.o1; out->o2 = t.o2;
  out->o1step = t.o1step; out->o2step = t.o2step;
  return IEM_OK;
}

int iem_kernel_info(const iem_model *m, int k, iem_kernel_info_t *out) {
  if (!m || !out || k < 0) return fail(IEM_E_ARG, "bad kernel index");
  // behind the model's own kernels: those of every derived program that exists on the handle (set up by its first call or
  // its prepare call), in the order of kDerived
  const iem::KernelDesc *found = k < (int)m->code.prog.kernels.size() ? &m->code.prog.kernels[k] : nullptr;
  int base = (int)m->code.prog.kernels.size();
  for (const LoadedProgram &P : m->derived) {
    if (found || !P.tried || P.rc != IEM_OK) continue;
    const int n = (int)P.prog.kernels.size();
    if (k < base + n) found = &P.prog.kernels[k - base];
    base += n;
  }
  if (!found) return fail(IEM_E_ARG, "bad kernel index");
  const iem::KernelDesc &kd = *found;
  std::memset(out, 0, sizeof *out);
  std::strncpy(out->name, kd.name.c_str(), sizeof(out->name) - 1);
  out->kind = kd.kind;
  for (int d = 0; d < 3; ++d) out->grid[d] = kd.grid[d];
  out->lds_bytes = kd.lds_bytes;
  out->alg_bytes_read = kd.alg_bytes_read;
  out->alg_bytes_written = kd.alg_bytes_written;
  out->jit = m->jit ? 1 : 0;
  return IEM_OK;
}

int iem_kernel_count(const iem_model *m, int32_t *out_total) {
  if (!m || !out_total) return fail(IEM_E_ARG, "null argument");
  size_t n = m->code.prog.kernels.size();
  for (const LoadedProgram &P : m->derived)
    if (P.tried && P.rc == IEM_OK) n += P.prog.kernels.size();
  *out_total = (int32_t)n;
  return IEM_OK;
}

int iem_get_host(const iem_model *m, int which, double *h_out) {
  if (!m || !h_out) return fail(IEM_E_ARG, "null argument");
  const iem::Model &M = m->model;
  switch (which) {
    case IEM_X0: case IEM_LVAR: case IEM_UVAR: {
      const iem::ArrayDesc &a = M.arrs[which == IEM_X0 ? M.arr_x0 : which == IEM_LVAR ? M.arr_lvar : M.arr_uvar];
      for (int64_t i = 0; i < M.nvar; ++i) h_out[i] = a.f(i);
      return IEM_OK;
    }
    case IEM_LCON: case IEM_UCON:
      for (const iem::Template &t : M.tpl) {
        if (t.kind != IEM_T_CON) continue;
        int mode = which == IEM_LCON ? t.lmode : t.umode;
        for (int64_t k = 0; k < t.n_items; ++k)
          h_out[t.o0 + k] = mode ? M.arrs[which == IEM_LCON ? t.larr : t.uarr].f(k) : (which == IEM_LCON ? t.lval : t.uval);
      }
      return IEM_OK;
    case IEM_Y0:
      for (int64_t i = 0; i < M.ncon; ++i) h_out[i] = 0.0;
      return IEM_OK;
    case IEM_THETA:
      std::memcpy(h_out, m->theta_host.data(), (size_t)M.npar * 8);
      return IEM_OK;
  }
  return fail(IEM_E_ARG, "unknown array selector");
}

int iem_set_stream(iem_model *m, void *hip_stream) {
  if (!m) return fail(IEM_E_ARG, "null handle");
  m->stream = (hipStream_t)hip_stream;
  return IEM_OK;
}

int iem_synchronize(iem_model *m) {
  if (!m) return fail(IEM_E_ARG, "null handle");
  DevGuard dg_(m->device);
  { int rc = halo_flush(m); if (rc) return rc; }   // a deferred exchange belongs to what the caller waits for
  HIP_TRY(hipStreamSynchronize(m->stream));
  return comm_check(m);
}

int iem_set_parameter(iem_model *m, int64_t off, int64_t len, const double *h_vals) {
  if (!m || !h_vals) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  if (off < 0 || len < 0 || off + len > m->model.npar) return fail(IEM_E_ARG, "parameter range out of bounds");
  std::memcpy(m->theta_host.data() + off, h_vals, (size_t)len * 8);
  HIP_TRY(hipMemcpyAsync(m->d_theta + off, m->theta_host.data() + off, (size_t)len * 8, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return IEM_OK;
}

int iem_obj_device(iem_model *m, const double *d_x, double *d_out) {
  if (!m || !d_x || !d_out) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  if (m->code.prog.n_partials == 0) {   // no objective template: f = 0
    HIP_TRY(hipMemsetAsync(d_out, 0, 8, m->stream));
    return IEM_OK;
  }
  LaunchHead h;   // the last workgroup of the objective kernel(s) to finish writes the scalar to aux
  h.x = d_x; h.out = m->code.d_partials; h.aux = d_out;
  return launch_kind(m, m->code, iem::KK_OBJ, h);
}

// The objective as a host scalar, in two halves (a solver that evaluates obj, grad!, cons!, jac_coord!, hess_coord! at one
// point — ext/InfiniteExaModelsIpopt.jl:48-49 — needs the VALUE only after the five launches are enqueued):
//   iem_obj_begin   arms the mapped host slot with a sentinel NaN and enqueues the objective kernel; returns at once
//   iem_obj_end     waits for the slot (polling, ~200 us, then a stream synchronise) and returns the value
// The last workgroup writes the scalar straight into mapped pinned host memory; the 8-byte store is atomic, so the first
// value that is not the sentinel is the result.  iem_obj = begin + end (the host round trip of one launch: ~14 us).
// Whatever fails after obj_arm disarms again, so that the next begin is not refused.
static const uint64_t kObjSentinel = 0x7ff8dead0bad0b1eULL;

static void obj_arm(iem_model *m) {
  *reinterpret_cast<volatile uint64_t *>(m->h_obj) = kObjSentinel;
  m->obj_armed = true;
  m->obj_scaled = false;   // (iem_eval_trial_scaled sets its factor behind its own arm)
}

int iem_obj_begin(iem_model *m, const double *d_x) {
  if (!m || !d_x) return fail(IEM_E_ARG, "null argument");
  if (m->obj_armed) return fail(IEM_E_ARG, "iem_obj_begin: the previous iem_obj_begin has not been collected (iem_obj_end)");
  obj_arm(m);
  if (m->code.prog.n_partials == 0) return IEM_OK;
  int rc = iem_obj_device(m, d_x, m->d_hobj);
  if (rc) m->obj_armed = false;
  return rc;
}

int iem_obj_end(iem_model *m, double *h_out) {
  if (!m || !h_out) return fail(IEM_E_ARG, "null argument");
  if (!m->obj_armed) return fail(IEM_E_ARG, "iem_obj_end without iem_obj_begin");
  m->obj_armed = false;
  const bool scaled = m->obj_scaled;   // the pending value is iem_eval_trial_scaled's: times its factor, one host multiply
  m->obj_scaled = false;
  if (m->code.prog.n_partials == 0) { *h_out = scaled ? m->obj_factor * 0.0 : 0.0; return comm_check(m); }
  DevGuard dg_(m->device);
  volatile uint64_t *slot = reinterpret_cast<volatile uint64_t *>(m->h_obj);
  bool got = false;
  if (m->poll_obj) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int spin = 0;; ++spin) {
      if (*slot != kObjSentinel) { got = true; break; }
      if ((spin & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) break;
    }
  }
  if (!got) HIP_TRY(hipStreamSynchronize(m->stream));   // large models, or a result that happens to BE the sentinel
  uint64_t bits = *slot;
  std::memcpy(h_out, &bits, 8);
  if (scaled) *h_out = m->obj_factor * *h_out;
  return comm_check(m);
}

int iem_obj(iem_model *m, const double *d_x, double *h_out) {
  if (!m || !h_out) return fail(IEM_E_ARG, "null argument");
  int rc = iem_obj_begin(m, d_x);
  if (rc) return rc;
  return iem_obj_end(m, h_out);
}

int iem_grad(iem_model *m, const double *d_x, double *d_g) {
  if (!m || !d_x || !d_g) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  LaunchHead h;
  h.x = d_x; h.out = d_g;
  return launch_scatter(m, m->code, iem::KK_GRAD, h);
}

/* NLPModels.jprod!(m, x, v, Jv) */
int iem_jprod(iem_model *m, const double *d_x, const double *d_v, double *d_Jv) {
  if (!m || !d_x || !d_v || (!d_Jv && m->model.ncon)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  LaunchHead h;
  h.x = d_x; h.v = d_v; h.out = d_Jv;
  return launch_kind(m, m->code, iem::KK_JPROD, h);
}

/* NLPModels.jtprod!(m, x, v, Jtv) */
int iem_jtprod(iem_model *m, const double *d_x, const double *d_v, double *d_Jtv) {
  if (!m || !d_x || (!d_v && m->model.ncon) || !d_Jtv) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  LaunchHead h;
  h.x = d_x; h.v = d_v; h.out = d_Jtv;
  return launch_scatter(m, m->code, iem::KK_JTPROD, h);
}

/* NLPModels.hprod!(m, x, y, v, Hv; obj_weight) */
int iem_hprod(iem_model *m, const double *d_x, const double *d_y, const double *d_v, double obj_weight, double *d_Hv) {
  if (!m || !d_x || (!d_y && m->model.ncon) || !d_v || !d_Hv) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  LaunchHead h;
  h.x = d_x; h.y = d_y; h.v = d_v; h.out = d_Hv; h.w = obj_weight;
  return launch_scatter(m, m->code, iem::KK_HPROD, h);
}

// ---- the derived programs ---------------------------------------------------------------------------------------------------
// One row per program of iem_model::derived, in the order of `Derived`.  `program`: the generator's program (iem_codegen.cpp:
// kPrograms), selected on top of the handle's own options.  `sharded`: why its entry points refuse a
// sharded handle.  `partials`: it has objective kernels, so it owns partials and ticket words.  To add a program: its row in
// kPrograms, a row here (and a name in `Derived`), its entry points, and a row in build().
struct DerivedRow {
  iem::ProgramId program;
  const char *sharded;
  bool partials;
};
static const char kShardedTheta[] = "θ is replicated on every rank, so the products with d/dθ would need an all-reduce over the ranks; "
                                    "sharded parameter products are out of scope";
static const DerivedRow kDerived[D_COUNT] = {
    // D_PAR: the three parameter kinds (iem_jpprod / iem_jptprod / iem_hpprod), shaped like jprod / jtprod / hprod
    {iem::PG_THETA, kShardedTheta, false},
    // D_ADJ: the adjoint parameter kind (iem_hptprod) on KK_HPROD's table slot
    {iem::PG_ADJOINT, kShardedTheta, false},
    // D_TH2: the θθ kind (iem_hppprod) on KK_HPROD's table slot
    {iem::PG_THETA2, kShardedTheta, false},
    // D_PC: the explicit θ blocks in COO (iem_jacp_coord on KK_JAC's table slot, iem_hessp_coord on KK_HESS's); no scatter kind
    {iem::PG_COORD, kShardedTheta, false},
    // D_LAG: the residual program (iem_lagrad / iem_eval_residual): lagrad on KK_JTPROD's table slot, the model's own cons and
    // obj, KK_TRIAL with lagrad as third member
    {iem::PG_LAGRAD,
     "the gradient of the Lagrangian would need the halo fold and the all-reduce of grad! and jtprod!; a sharded residual is out of scope", true},
    // D_SCL: the scaled program (iem_jac_rowmax / iem_cons_scaled / iem_jac_coord_scaled): rowmax on KK_JPROD's table slot,
    // cons_scaled on KK_CONS's, jac_scaled on KK_JAC's; s = the head's v.  No scatter kind: no follow-up, no memset
    {iem::PG_SCALED,
     "the values need no communication, but the deferred halo exchange (carrier workgroup, flush in front of a launch that reads a halo entry) "
     "is not taught this program; scaled kernels on a sharded handle are out of scope", false},
    // D_KKT: the KKT operator (iem_kktprod): kktx on KK_HPROD's table slot, kkty on KK_JPROD's, KK_TRIAL with both as members;
    // u = the head's v, the dual direction = the head's last word
    {iem::PG_KKT,
     "the x-part would need the halo fold and the all-reduce of hprod! and jtprod!; a sharded KKT operator is out of scope", false},
    // D_SPH: the scaled solver phases (iem_eval_trial_scaled / iem_eval_accepted_scaled and their members): sp_cons / sp_jac /
    // sp_hess / sp_obj / sp_grad on the model's own table slots, KK_TRIAL and KK_ACCEPTED over them; s = the head's v, y = the head's y
    {iem::PG_SPHASE,
     "the scaled gradient would need the halo fold and the all-reduce of grad!, and the deferred halo exchange is not taught this program; "
     "scaled solver phases on a sharded handle are out of scope", true},
};

static int sharded_refusal(const iem_model *m, Derived d, const char *what) {
  if (!m->sharded) return IEM_OK;
  return fail(IEM_E_ARG, std::string(what) + ": not available on a sharded handle — " + kDerived[d].sharded);
}

// The derived program `d` of the handle, generated and loaded by the first call that needs it (code-object cache -> hiprtc
// on a miss, like the model's own).  A model the generator refuses stays refused, and every later call reports that; a runtime
// failure (out of memory, a compile that did not go through) is not remembered: what was set up is released and the next
// call tries again.
static int derived_program(iem_model *m, Derived d) {
  LoadedProgram &P = m->derived[d];
  if (P.tried) return P.rc ? fail(P.rc, P.err) : IEM_OK;
  iem::Options po = m->opt;
  iem::select_program(po, kDerived[d].program);
  int rc = IEM_OK;
  try {
    P.prog = iem::generate(m->model, po);
  } catch (const std::exception &e) {
    rc = fail(IEM_E_BLOB, e.what());
  }
  // (a program without a kernel — no mixed / no θθ term at all: hptprod / hppprod is the runtime's memset — has no code object)
  if (rc == IEM_OK && !P.prog.kernels.empty() && (rc = load_program(m, P, po)) == IEM_OK && (rc = scatter_buffers(P, &m->stream)) == IEM_OK)
    rc = prepare_program(m, P);
  if (rc == IEM_OK && kDerived[d].partials) rc = partials_buffer(P, &m->stream);
  if (rc != IEM_OK && rc != IEM_E_BLOB) {
    release_program(P);
    return rc;
  }
  for (int kind = 0; kind < iem::KK_COUNT; ++kind) P.zero_ranges[kind] = P.prog.zero_ranges[kind];
  P.tried = true;
  P.rc = rc;
  if (rc) P.err = g_err;
  return rc;
}

// the prepare entry points: the programs `first` .. `last` set up, the number of their kernels out
static int derived_prepare(iem_model *m, const char *what, Derived first, Derived last, int32_t *out_n_kernels) {
  if (!m) return fail(IEM_E_ARG, "null handle");
  int rc = sharded_refusal(m, first, what);
  if (rc) return rc;
  DevGuard dg_(m->device);
  size_t n = 0;
  for (int d = first; d <= last; ++d) {
    if ((rc = derived_program(m, (Derived)d))) return rc;
    n += m->derived[d].prog.kernels.size();
  }
  if (out_n_kernels) *out_n_kernels = (int32_t)n;
  return IEM_OK;
}

int iem_param_prepare(iem_model *m, int32_t *out_n_kernels) { return derived_prepare(m, "iem_param_prepare", D_PAR, D_ADJ, out_n_kernels); }
int iem_hppprod_prepare(iem_model *m, int32_t *out_n_kernels) { return derived_prepare(m, "iem_hppprod_prepare", D_TH2, D_TH2, out_n_kernels); }
int iem_param_coord_prepare(iem_model *m, int32_t *out_n_kernels) { return derived_prepare(m, "iem_param_coord_prepare", D_PC, D_PC, out_n_kernels); }
int iem_lagrad_prepare(iem_model *m, int32_t *out_n_kernels) { return derived_prepare(m, "iem_lagrad_prepare", D_LAG, D_LAG, out_n_kernels); }
int iem_scaled_prepare(iem_model *m, int32_t *out_n_kernels) { return derived_prepare(m, "iem_scaled_prepare", D_SCL, D_SCL, out_n_kernels); }
int iem_scaled_phase_prepare(iem_model *m, int32_t *out_n_kernels) { return derived_prepare(m, "iem_scaled_phase_prepare", D_SPH, D_SPH, out_n_kernels); }

// ---- parameter sensitivities: products with d/dθ at (x, the handle's current θ) ------------------------------------------
int iem_jpprod(iem_model *m, const double *d_x, const double *d_w, double *d_out) {
  if (!m || !d_x || (!d_w && m->model.npar) || (!d_out && m->model.ncon)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_PAR, "iem_jpprod");
  if (rc) return rc;
  DevGuard dg_(m->device);
  if (m->model.ncon == 0) return IEM_OK;
  if ((rc = derived_program(m, D_PAR))) return rc;
  LaunchHead h;
  h.x = d_x; h.v = d_w; h.out = d_out;
  return launch_kind(m, m->derived[D_PAR], iem::KK_JPROD, h);
}

int iem_jptprod(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_out) {
  if (!m || !d_x || (!d_y && m->model.ncon) || (!d_out && m->model.npar)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_PAR, "iem_jptprod");
  if (rc) return rc;
  if (m->model.npar == 0) return IEM_OK;   // a zero-length output: nothing to launch
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_PAR))) return rc;
  LaunchHead h;
  h.x = d_x; h.v = d_y; h.out = d_out; h.w = obj_weight;
  return launch_scatter(m, m->derived[D_PAR], iem::KK_JTPROD, h);
}

int iem_hpprod(iem_model *m, const double *d_x, const double *d_y, double obj_weight, const double *d_w, double *d_out) {
  if (!m || !d_x || (!d_y && m->model.ncon) || (!d_w && m->model.npar) || (!d_out && m->model.nvar)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_PAR, "iem_hpprod");
  if (rc) return rc;
  DevGuard dg_(m->device);
  if (m->model.nvar == 0) return IEM_OK;
  if ((rc = derived_program(m, D_PAR))) return rc;
  LaunchHead h;
  h.x = d_x; h.y = d_y; h.v = d_w; h.out = d_out; h.w = obj_weight;
  return launch_scatter(m, m->derived[D_PAR], iem::KK_HPROD, h);
}

int iem_hptprod(iem_model *m, const double *d_x, const double *d_y, double obj_weight, const double *d_u, double *d_out) {
  if (!m || !d_x || (!d_y && m->model.ncon) || (!d_u && m->model.nvar) || (!d_out && m->model.npar)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_ADJ, "iem_hptprod");
  if (rc) return rc;
  if (m->model.npar == 0) return IEM_OK;   // a zero-length output: nothing to launch
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_ADJ))) return rc;
  LaunchHead h;
  h.x = d_x; h.y = d_y; h.v = d_u; h.out = d_out; h.w = obj_weight;
  return launch_scatter(m, m->derived[D_ADJ], iem::KK_HPROD, h);
}

int iem_hppprod(iem_model *m, const double *d_x, const double *d_y, double obj_weight, const double *d_w, double *d_out) {
  if (!m || !d_x || (!d_y && m->model.ncon) || ((!d_w || !d_out) && m->model.npar)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_TH2, "iem_hppprod");
  if (rc) return rc;
  if (m->model.npar == 0) return IEM_OK;   // a zero-length output: nothing to launch
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_TH2))) return rc;
  LaunchHead h;
  h.x = d_x; h.y = d_y; h.v = d_w; h.out = d_out; h.w = obj_weight;
  return launch_scatter(m, m->derived[D_TH2], iem::KK_HPROD, h);
}

// ---- the blocks themselves in COO: dc/dθ, d2L/dx dθ, d2L/dθ2 at (x, the handle's current θ) ------------------------------
// Slot order (the structure calls are the authority): template order, within a template item ordinal times kept slots per
// item, within an item the order of the parameter view's first- / second-order slot lists.  The pattern is symbolic.
static const iem::Model &param_coord_view(iem_model *m) {
  if (!m->pc_have_view) {
    m->pc_view = iem::parameter_view(m->model);
    iem::param_coord_layout(m->pc_view);
    m->pc_have_view = true;
  }
  return m->pc_view;
}

int iem_param_coord_nnz(iem_model *m, int64_t out[3]) {
  if (!m || !out) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_PC, "iem_param_coord_nnz");
  if (rc) return rc;
  const iem::Model &v = param_coord_view(m);
  out[0] = v.nnzjp; out[1] = v.nnzhxp; out[2] = v.nnzhpp;
  return IEM_OK;
}

static int param_coord_structure(iem_model *m, int which, int64_t *h_rows, int64_t *h_cols, int base, const char *what) {
  if (!m) return fail(IEM_E_ARG, "null handle");
  int rc = sharded_refusal(m, D_PC, what);
  if (rc) return rc;
  const iem::Model &v = param_coord_view(m);
  const int64_t n = which == 0 ? v.nnzjp : which == 1 ? v.nnzhxp : v.nnzhpp;
  if ((!h_rows || !h_cols) && n) return fail(IEM_E_ARG, "null argument");
  param_coord_structure_host(v, which, h_rows, h_cols, base);
  return IEM_OK;
}

int iem_jacp_structure(iem_model *m, int64_t *h_rows, int64_t *h_cols, int base) { return param_coord_structure(m, 0, h_rows, h_cols, base, "iem_jacp_structure"); }
int iem_hessxp_structure(iem_model *m, int64_t *h_rows, int64_t *h_cols, int base) { return param_coord_structure(m, 1, h_rows, h_cols, base, "iem_hessxp_structure"); }
int iem_hesspp_structure(iem_model *m, int64_t *h_rows, int64_t *h_cols, int base) { return param_coord_structure(m, 2, h_rows, h_cols, base, "iem_hesspp_structure"); }

int iem_jacp_coord(iem_model *m, const double *d_x, double *d_vals) {
  if (!m || !d_x) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_PC, "iem_jacp_coord");
  if (rc) return rc;
  if (param_coord_view(m).nnzjp == 0) return IEM_OK;   // no θ slot in any constraint: nothing to launch
  if (!d_vals) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_PC))) return rc;
  LaunchHead h;
  h.x = d_x; h.out = d_vals;
  return launch_kind(m, m->derived[D_PC], iem::KK_JAC, h);
}

int iem_hessp_coord(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_hessxp, double *d_hesspp) {
  if (!m || !d_x || (!d_y && m->model.ncon)) return fail(IEM_E_ARG, "null argument");
  if (!d_hessxp && !d_hesspp) return fail(IEM_E_ARG, "iem_hessp_coord: both outputs are NULL");
  int rc = sharded_refusal(m, D_PC, "iem_hessp_coord");
  if (rc) return rc;
  const iem::Model &v = param_coord_view(m);
  if (v.nnzhxp == 0 && v.nnzhpp == 0) return IEM_OK;   // no second-order slot touches θ: nothing to launch
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_PC))) return rc;
  // both blocks come out of ONE sweep: a block the caller does not want (NULL) but that has entries goes to a spare buffer
  double *outp[2] = {d_hessxp, d_hesspp};
  const int64_t nn[2] = {v.nnzhxp, v.nnzhpp};
  for (int b = 0; b < 2; ++b) {
    if (outp[b] || nn[b] == 0) continue;
    if (!m->d_pc_spare[b]) HIP_TRY(hipMalloc((void **)&m->d_pc_spare[b], (size_t)nn[b] * 8));
    outp[b] = m->d_pc_spare[b];
  }
  LaunchHead h;
  h.x = d_x; h.y = d_y; h.w = obj_weight; h.out = outp[0]; h.aux = outp[1];
  return launch_kind(m, m->derived[D_PC], iem::KK_HESS, h);
}

// ---- the convergence check: the Lagrangian's gradient in one kernel, c, f and that gradient in one launch ------------------
/* σ ∇f(x) + J(x)' y — the dual residual of a solver's convergence check, without the bound multipliers */
int iem_lagrad(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_out) {
  if (!m || !d_x || (!d_y && m->model.ncon) || (!d_out && m->model.nvar)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_LAG, "iem_lagrad");
  if (rc) return rc;
  if (m->model.nvar == 0) return IEM_OK;   // a zero-length output: nothing to launch
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_LAG))) return rc;
  LaunchHead h;
  h.x = d_x; h.v = d_y; h.out = d_out; h.w = obj_weight;
  return launch_scatter(m, m->derived[D_LAG], iem::KK_JTPROD, h);   // (no first-order slot at all: the zero range is the whole output, a memset)
}

/* c(x), f(x) and the gradient above in ONE launch (the residual program's KK_TRIAL), lagrad's follow-ups behind it; where
 * that kernel does not exist (no objective, no constraint or no first-order slot; kinds of different workgroup sizes; more
 * workgroups than one launch takes) the member launches */
int iem_eval_residual(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_c, double *d_lagrad, double *d_obj) {
  if (!m || !d_x || !d_obj || ((!d_y || !d_c) && m->model.ncon) || (!d_lagrad && m->model.nvar)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_LAG, "iem_eval_residual");
  if (rc) return rc;
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_LAG))) return rc;
  LoadedProgram &P = m->derived[D_LAG];
  LaunchHead h;
  h.x = d_x; h.v = d_y; h.w = obj_weight;
  if (!P.launchable[iem::KK_TRIAL].empty()) {
    if ((rc = zero_uncovered(m, P, iem::KK_JTPROD, d_lagrad))) return rc;
    h.out = d_c; h.aux = d_obj; h.trial_partials = P.d_partials; h.lag_out = d_lagrad; h.lag_red = P.d_red[iem::KK_JTPROD];
    if ((rc = launch_kind(m, P, iem::KK_TRIAL, h))) return rc;
    return kind_followups(m, P, iem::KK_JTPROD, h.lag_out, h.lag_red);
  }
  h.out = d_c;
  if ((rc = launch_kind(m, P, iem::KK_CONS, h))) return rc;
  if (P.launchable[iem::KK_OBJ].empty()) {   // no objective template: f = 0
    HIP_TRY(hipMemsetAsync(d_obj, 0, 8, m->stream));
  } else {
    h.out = P.d_partials; h.aux = d_obj;
    if ((rc = launch_kind(m, P, iem::KK_OBJ, h))) return rc;
  }
  if (m->model.nvar == 0) return IEM_OK;
  h.out = d_lagrad;
  return launch_scatter(m, P, iem::KK_JTPROD, h);
}

// ---- row scaling in the kernels: the row maxima of the Jacobian, scaled cons! and scaled jac_coord! -------------------------
/* max over the first-order slots of row r of |dc_r/dx_slot| (repeated positions not summed; 0 for a row without a slot; NaN stays) */
int iem_jac_rowmax(iem_model *m, const double *d_x, double *d_rowmax) {
  if (!m || !d_x || (!d_rowmax && m->model.ncon)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_SCL, "iem_jac_rowmax");
  if (rc) return rc;
  if (m->model.ncon == 0) return IEM_OK;   // a zero-length output: nothing to launch
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_SCL))) return rc;
  LaunchHead h;
  h.x = d_x; h.out = d_rowmax;
  return launch_kind(m, m->derived[D_SCL], iem::KK_JPROD, h);
}

/* s[r] * c_r(x) */
int iem_cons_scaled(iem_model *m, const double *d_x, const double *d_s, double *d_c) {
  if (!m || !d_x || ((!d_s || !d_c) && m->model.ncon)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_SCL, "iem_cons_scaled");
  if (rc) return rc;
  if (m->model.ncon == 0) return IEM_OK;
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_SCL))) return rc;
  LaunchHead h;
  h.x = d_x; h.v = d_s; h.out = d_c;
  return launch_kind(m, m->derived[D_SCL], iem::KK_CONS, h);
}

/* s[row(k)] * jac[k] at the positions of iem_jac_structure */
int iem_jac_coord_scaled(iem_model *m, const double *d_x, const double *d_s, double *d_vals) {
  if (!m || !d_x || (!d_s && m->model.ncon) || (!d_vals && m->model.nnzj)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_SCL, "iem_jac_coord_scaled");
  if (rc) return rc;
  if (m->model.nnzj == 0) return IEM_OK;
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_SCL))) return rc;
  LaunchHead h;
  h.x = d_x; h.v = d_s; h.out = d_vals;
  return launch_kind(m, m->derived[D_SCL], iem::KK_JAC, h);
}

// ---- the KKT operator: out_x = W u + J' v, out_y = J u in one launch ----------------------------------------------------------
// kktx's memsets and follow-ups stay here, as lagrad's do.
static int kkt_zero_direction(iem_model *m) {
  if (!m->d_kkt_zero && m->model.ncon > 0) {   // the dual direction of a call with d_v == NULL
    const size_t bytes = (size_t)m->model.ncon * 8;
    if (hipMalloc((void **)&m->d_kkt_zero, bytes) != hipSuccess) { m->d_kkt_zero = nullptr; return fail(IEM_E_HIP, "hipMalloc zero direction"); }
    if (hipMemset(m->d_kkt_zero, 0, bytes) != hipSuccess) { hipFree(m->d_kkt_zero); m->d_kkt_zero = nullptr; return fail(IEM_E_HIP, "hipMemset zero direction"); }
  }
  return IEM_OK;
}

int iem_kktprod_prepare(iem_model *m, int32_t *out_n_kernels) {
  int rc = derived_prepare(m, "iem_kktprod_prepare", D_KKT, D_KKT, out_n_kernels);
  if (rc) return rc;
  DevGuard dg_(m->device);
  return kkt_zero_direction(m);   // (so that a prepared handle allocates nothing in iem_kktprod)
}

static bool kkt_overlap(const double *a, int64_t na, const double *b, int64_t nb) {
  if (!a || !b || na <= 0 || nb <= 0) return false;
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * 8, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * 8;
  return a0 < b1 && b0 < a1;
}

int iem_kktprod(iem_model *m, const double *d_x, const double *d_y, double obj_weight, const double *d_u, const double *d_v, double *d_out_x, double *d_out_y) {
  if (!m) return fail(IEM_E_ARG, "null argument");
  const int64_t nvar = m->model.nvar, ncon = m->model.ncon;
  if (((!d_x || !d_u || !d_out_x) && nvar) || ((!d_y || !d_out_y) && ncon)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_KKT, "iem_kktprod");
  if (rc) return rc;
  for (const auto &in : {std::make_pair(d_x, nvar), std::make_pair(d_u, nvar), std::make_pair(d_y, ncon), std::make_pair(d_v, ncon)})
    if (kkt_overlap(d_out_x, nvar, in.first, in.second) || kkt_overlap(d_out_y, ncon, in.first, in.second))
      return fail(IEM_E_ARG, "iem_kktprod: an output overlaps an input");
  if (kkt_overlap(d_out_x, nvar, d_out_y, ncon)) return fail(IEM_E_ARG, "iem_kktprod: the two outputs overlap");
  if (nvar == 0 && ncon == 0) return IEM_OK;
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_KKT)) || (rc = kkt_zero_direction(m))) return rc;
  LoadedProgram &P = m->derived[D_KKT];
  LaunchHead h;
  h.x = d_x; h.y = d_y; h.v = d_u; h.w = obj_weight;
  h.obj = const_cast<double *>(d_v ? d_v : m->d_kkt_zero);   // (the head's last word: read only)
  double *red = P.d_red[iem::KK_HPROD];
  if (nvar && (rc = zero_uncovered(m, P, iem::KK_HPROD, d_out_x))) return rc;
  if (!P.launchable[iem::KK_TRIAL].empty()) {
    h.out = d_out_x; h.aux = red; h.g = d_out_y;
    if ((rc = launch_kind(m, P, iem::KK_TRIAL, h))) return rc;
    return kind_followups(m, P, iem::KK_HPROD, d_out_x, red);
  }
  h.out = d_out_y;
  if ((rc = launch_kind(m, P, iem::KK_JPROD, h))) return rc;
  if (nvar == 0) return IEM_OK;
  h.out = d_out_x; h.aux = red;
  return launch_kind(m, P, iem::KK_HPROD, h);
}

// ---- one launch per solver phase for the SCALED NLP ---------------------------------------------------------------------------
// The accepted phase has two scalars: the head's w is the Hessian's objective weight, the gradient's seed travels as the bits
// of a double in the head's word p4.  sp_grad's memsets and follow-ups stay here.
/* obj_scale * grad f(x): the reverse sweep seeded with obj_scale */
int iem_grad_scaled(iem_model *m, const double *d_x, double obj_scale, double *d_g) {
  if (!m || !d_x || (!d_g && m->model.nvar)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_SPH, "iem_grad_scaled");
  if (rc) return rc;
  if (m->model.nvar == 0) return IEM_OK;
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_SPH))) return rc;
  LaunchHead h;
  h.x = d_x; h.out = d_g; h.w = obj_scale;
  return launch_scatter(m, m->derived[D_SPH], iem::KK_GRAD, h);   // (the memset is the whole of g on a model without an objective)
}

/* hess_coord!(x, fl(y∘s); obj_weight): the multiplier of a scaled row formed in the kernel */
int iem_hess_coord_scaled(iem_model *m, const double *d_x, const double *d_y, const double *d_s, double obj_weight, double *d_vals) {
  if (!m || !d_x || ((!d_y || !d_s) && m->model.ncon) || (!d_vals && m->model.nnzh)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_SPH, "iem_hess_coord_scaled");
  if (rc) return rc;
  if (m->model.nnzh == 0) return IEM_OK;
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_SPH))) return rc;
  LaunchHead h;
  h.x = d_x; h.y = d_y; h.v = d_s; h.out = d_vals; h.w = obj_weight;
  return launch_kind(m, m->derived[D_SPH], iem::KK_HESS, h);
}

/* s∘cons(x) and obj_scale·obj(x) in ONE launch (the program's KK_TRIAL); where that kernel does not exist (option
 * "phase_kernels" = 0, no objective or no constraint, more workgroups than one launch takes) the member launches */
int iem_eval_trial_scaled(iem_model *m, const double *d_x, const double *d_s, double obj_scale, double *d_c, double *h_obj) {
  if (!m || !d_x || ((!d_s || !d_c) && m->model.ncon)) return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_SPH, "iem_eval_trial_scaled");
  if (rc) return rc;
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_SPH))) return rc;
  if (m->obj_armed) return fail(IEM_E_ARG, "iem_eval_trial_scaled: the previous iem_obj_begin / iem_eval_trial has not been collected (iem_obj_end)");
  LoadedProgram &P = m->derived[D_SPH];
  obj_arm(m);
  m->obj_scaled = true; m->obj_factor = obj_scale;
  LaunchHead h;   // the kernel writes the model's own f into the mapped slot, the factor meets it on the host (iem_obj_end)
  h.x = d_x; h.v = d_s;
  if (!P.launchable[iem::KK_TRIAL].empty()) {
    h.out = d_c; h.aux = m->d_hobj; h.trial_partials = P.d_partials;
    rc = launch_kind(m, P, iem::KK_TRIAL, h);
  } else {
    h.out = d_c;
    rc = launch_kind(m, P, iem::KK_CONS, h);
    if (rc == IEM_OK) {   // (no objective template: nothing is launched and iem_obj_end gives 0)
      h.out = P.d_partials; h.aux = m->d_hobj;
      rc = launch_kind(m, P, iem::KK_OBJ, h);
    }
  }
  if (rc) { m->obj_armed = false; m->obj_scaled = false; return rc; }
  return h_obj ? iem_obj_end(m, h_obj) : IEM_OK;
}

/* obj_scale·grad f, s[row]·jac and hess_coord!(x, fl(y∘s); fl(obj_weight·obj_scale)) in ONE launch (the program's
 * KK_ACCEPTED), sp_grad's follow-ups behind it; where that kernel does not exist, the member launches */
int iem_eval_accepted_scaled(iem_model *m, const double *d_x, const double *d_y, const double *d_s, double obj_scale, double obj_weight,
                             double *d_g, double *d_jac, double *d_hess) {
  if (!m || !d_x || (!d_g && m->model.nvar) || ((!d_y || !d_s) && m->model.ncon) || (!d_jac && m->model.nnzj) || (!d_hess && m->model.nnzh))
    return fail(IEM_E_ARG, "null argument");
  int rc = sharded_refusal(m, D_SPH, "iem_eval_accepted_scaled");
  if (rc) return rc;
  DevGuard dg_(m->device);
  if ((rc = derived_program(m, D_SPH))) return rc;
  LoadedProgram &P = m->derived[D_SPH];
  const double w = obj_weight * obj_scale;   // the Hessian's objective weight as used: one host multiply
  if (m->model.nvar && (rc = zero_uncovered(m, P, iem::KK_GRAD, d_g))) return rc;
  LaunchHead h;
  h.x = d_x; h.y = d_y; h.v = d_s; h.w = w;
  if (!P.launchable[iem::KK_ACCEPTED].empty()) {
    h.out = d_jac; h.aux = d_hess; h.g = d_g; h.g_red = P.d_red[iem::KK_GRAD];
    static_assert(sizeof h.c == sizeof obj_scale, "the gradient's seed rides on one word of the head");
    std::memcpy(&h.c, &obj_scale, 8);   // (the head's p4: the bits of sp_grad's seed, iem_sp_word)
    if ((rc = launch_kind(m, P, iem::KK_ACCEPTED, h))) return rc;
    return kind_followups(m, P, iem::KK_GRAD, h.g, h.g_red);
  }
  h.out = d_jac;
  if ((rc = launch_kind(m, P, iem::KK_JAC, h))) return rc;
  h.out = d_hess;
  if ((rc = launch_kind(m, P, iem::KK_HESS, h))) return rc;
  if (m->model.nvar == 0) return IEM_OK;
  h.out = d_g; h.w = obj_scale; h.aux = P.d_red[iem::KK_GRAD];
  return launch_kind(m, P, iem::KK_GRAD, h);
}

int iem_cons(iem_model *m, const double *d_x, double *d_c) {
  if (!m || !d_x || (!d_c && m->model.ncon)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  LaunchHead h;
  h.x = d_x; h.out = d_c;
  return launch_kind(m, m->code, iem::KK_CONS, h);
}

int iem_jac_coord(iem_model *m, const double *d_x, double *d_vals) {
  if (!m || !d_x || (!d_vals && m->model.nnzj)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  LaunchHead h;
  h.x = d_x; h.out = d_vals;
  return launch_tuned(m, 0, iem::KK_JAC, h);
}

int iem_hess_coord(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_vals) {
  if (!m || !d_x || (!d_y && m->model.ncon) || (!d_vals && m->model.nnzh)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  LaunchHead h;
  h.x = d_x; h.y = d_y; h.out = d_vals; h.w = obj_weight;
  return launch_tuned(m, 1, iem::KK_HESS, h);
}

/* jac_coord!(m, x, jac) and hess_coord!(m, x, y, hess; obj_weight) in ONE launch (kernel kind KK_PAIR): the two calls are
 * independent given x and y, so their workgroups share a launch — one ramp and one drain, and on a shard-sized grid both
 * kinds are resident together.  Identical bytes to the two separate calls.  Handles without a launchable fused kernel
 * (option "pair_kernel" = 0, or only one of the two kinds exists) make the two calls. */
int iem_jac_hess_coord(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_jac, double *d_hess) {
  if (!m || !d_x || (!d_y && m->model.ncon) || (!d_jac && m->model.nnzj) || (!d_hess && m->model.nnzh)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  if (!m->code.launchable[iem::KK_PAIR].empty()) {
    LaunchHead h;
    h.x = d_x; h.y = d_y; h.out = d_jac; h.w = obj_weight; h.aux = d_hess;
    return launch_kind(m, m->code, iem::KK_PAIR, h);
  }
  int rc = iem_jac_coord(m, d_x, d_jac);
  if (rc == IEM_OK) rc = iem_hess_coord(m, d_x, d_y, obj_weight, d_hess);
  return rc;
}

/* One launch per solver phase (kernel kinds KK_TRIAL / KK_ACCEPTED): an interior-point solver evaluates obj + cons! at every
 * TRIAL point of its line search and grad! + jac_coord! + hess_coord! once per ACCEPTED point (the reference's solvers:
 * ext/InfiniteExaModelsMadNLP.jl:49-50,64, ext/InfiniteExaModelsIpopt.jl:48-49).  The member kinds' bodies — the very
 * functions the separate calls run — sit behind one workgroup-id dispatcher: identical bytes, one launch instead of two /
 * three (5-7 us each on the grids the reference benchmarks, ESCAPE34/run_cases_gpu.jl:89-102).  Handles without a launchable
 * kernel (option "phase_kernels" = 0, a model without objective or without constraints, kinds of different workgroup sizes)
 * make the separate calls. */
int iem_eval_trial(iem_model *m, const double *d_x, double *d_c, double *h_obj) {
  if (!m || !d_x || (!d_c && m->model.ncon)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  int rc;
  if (!m->code.launchable[iem::KK_TRIAL].empty() && m->code.prog.n_partials > 0) {
    if (m->obj_armed) return fail(IEM_E_ARG, "iem_eval_trial: the previous iem_obj_begin / iem_eval_trial has not been collected (iem_obj_end)");
    obj_arm(m);
    LaunchHead h;
    h.x = d_x; h.out = d_c; h.aux = m->d_hobj; h.trial_partials = m->code.d_partials;
    rc = launch_kind(m, m->code, iem::KK_TRIAL, h);
  } else if ((rc = iem_obj_begin(m, d_x)) == IEM_OK) {
    rc = iem_cons(m, d_x, d_c);
  } else {
    return rc;   // (not armed)
  }
  if (rc) { m->obj_armed = false; return rc; }
  return h_obj ? iem_obj_end(m, h_obj) : IEM_OK;
}

int iem_eval_accepted(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_g, double *d_jac, double *d_hess) {
  if (!m || !d_x || !d_g || (!d_y && m->model.ncon) || (!d_jac && m->model.nnzj) || (!d_hess && m->model.nnzh)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  if (!m->code.launchable[iem::KK_ACCEPTED].empty()) {
    int rc = zero_uncovered(m, m->code, iem::KK_GRAD, d_g);
    if (rc) return rc;
    LaunchHead h;
    h.x = d_x; h.y = d_y; h.out = d_jac; h.w = obj_weight; h.aux = d_hess; h.g = d_g; h.g_red = m->code.d_red[iem::KK_GRAD];
    if ((rc = launch_kind(m, m->code, iem::KK_ACCEPTED, h))) return rc;
    return kind_followups(m, m->code, iem::KK_GRAD, h.g, h.g_red);
  }
  int rc = iem_grad(m, d_x, d_g);
  if (rc == IEM_OK) rc = iem_jac_hess_coord(m, d_x, d_y, obj_weight, d_jac, d_hess);
  return rc;
}

/* obj, cons!, grad!, jac_coord!, hess_coord! of ONE point in ONE launch (kernel kind KK_ALL): the five evaluations a solver
 * makes when its first trial point is accepted.  h_obj as in iem_eval_trial. */
int iem_eval_all(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_c, double *d_g, double *d_jac, double *d_hess,
                 double *h_obj) {
  if (!m || !d_x || !d_g || (!d_c && m->model.ncon) || (!d_y && m->model.ncon) || (!d_jac && m->model.nnzj) || (!d_hess && m->model.nnzh))
    return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  int rc;
  if (!m->code.launchable[iem::KK_ALL].empty() && m->code.prog.n_partials > 0) {
    if (m->obj_armed) return fail(IEM_E_ARG, "iem_eval_all: the previous iem_obj_begin / iem_eval_trial / iem_eval_all has not been collected (iem_obj_end)");
    if ((rc = zero_uncovered(m, m->code, iem::KK_GRAD, d_g))) return rc;
    obj_arm(m);
    LaunchHead h;
    h.x = d_x; h.y = d_y; h.out = d_jac; h.w = obj_weight; h.aux = d_hess; h.g = d_g; h.g_red = m->code.d_red[iem::KK_GRAD];
    h.c = d_c; h.partials = m->code.d_partials; h.obj = m->d_hobj;
    if ((rc = launch_kind(m, m->code, iem::KK_ALL, h)) == IEM_OK) rc = kind_followups(m, m->code, iem::KK_GRAD, h.g, h.g_red);
  } else if ((rc = iem_eval_trial(m, d_x, d_c, nullptr)) == IEM_OK) {
    rc = iem_eval_accepted(m, d_x, d_y, obj_weight, d_g, d_jac, d_hess);
  } else {
    return rc;   // (not armed)
  }
  if (rc) { m->obj_armed = false; return rc; }
  return h_obj ? iem_obj_end(m, h_obj) : IEM_OK;
}

int iem_jac_structure(iem_model *m, int64_t *h_rows, int64_t *h_cols, int base) {
  if (!m || ((!h_rows || !h_cols) && m->model.nnzj)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  jac_structure_host(m->model, h_rows, h_cols, base);
  return IEM_OK;
}

int iem_hess_structure(iem_model *m, int64_t *h_rows, int64_t *h_cols, int base) {
  if (!m || ((!h_rows || !h_cols) && m->model.nnzh)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  if (!m->code.prog.hess_classes.empty()) hess_structure_merged_host(m->model, m->code.prog.hess_classes, h_rows, h_cols, base);
  else hess_structure_host(m->model, h_rows, h_cols, base);
  return IEM_OK;
}

int iem_jac_structure_device(iem_model *m, int64_t *d_rows, int64_t *d_cols, int base) {
  if (!m || ((!d_rows || !d_cols) && m->model.nnzj)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  return structure_device(m, d_rows, d_cols, base, false);
}

int iem_hess_structure_device(iem_model *m, int64_t *d_rows, int64_t *d_cols, int base) {
  if (!m || ((!d_rows || !d_cols) && m->model.nnzh)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(m->device);
  return structure_device(m, d_rows, d_cols, base, true);
}

int iem_csr_values(iem_model *m, int64_t n_csr, const int64_t *d_seg, const int64_t *d_perm, const double *d_coo,
                   double *d_csr) {
  if (!m || n_csr < 0 || (n_csr && (!d_seg || !d_perm || !d_coo || !d_csr))) return fail(IEM_E_ARG, "bad argument");
  DevGuard dg_(m->device);
  if (n_csr == 0) return IEM_OK;
  long long n = n_csr;
  void *args[] = {(void *)&d_seg, (void *)&d_perm, (void *)&d_coo, (void *)&d_csr, (void *)&n};
  HIP_TRY(hipModuleLaunchKernel(m->fn_csr, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, m->stream, args, nullptr));
  return IEM_OK;
}

int iem_csr_values32(iem_model *m, int64_t n_csr, const uint32_t *d_seg, const uint32_t *d_perm, const double *d_coo,
                     double *d_csr) {
  if (!m || n_csr < 0 || (n_csr && (!d_seg || !d_perm || !d_coo || !d_csr))) return fail(IEM_E_ARG, "bad argument");
  DevGuard dg_(m->device);
  if (n_csr == 0) return IEM_OK;
  long long n = n_csr;
  void *args[] = {(void *)&d_seg, (void *)&d_perm, (void *)&d_coo, (void *)&d_csr, (void *)&n};
  HIP_TRY(hipModuleLaunchKernel(m->fn_csr32, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, m->stream, args, nullptr));
  return IEM_OK;
}

int iem_csr_spmv(iem_model *m, int64_t n, const int32_t *d_rowptr, const int32_t *d_colind, const double *d_vals, const double *d_x, double *d_y,
                 int64_t n_long, const int64_t *d_long_rows) {
  if (!m || n < 0 || n_long < 0 || (n && (!d_rowptr || !d_colind || !d_vals || !d_x || !d_y)) || (n_long && !d_long_rows)) return fail(IEM_E_ARG, "bad argument");
  DevGuard dg_(m->device);
  if (n == 0) return IEM_OK;
  long long nn = n;
  int skip = n_long > 0 ? IEM_SPMV_LONG_ROW : 0;
  void *args[] = {(void *)&d_rowptr, (void *)&d_colind, (void *)&d_vals, (void *)&d_x, (void *)&d_y, (void *)&nn, (void *)&skip};
  HIP_TRY(hipModuleLaunchKernel(m->fn_spmv, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, m->stream, args, nullptr));
  if (n_long > 0) {
    void *largs[] = {(void *)&d_rowptr, (void *)&d_colind, (void *)&d_vals, (void *)&d_x, (void *)&d_y, (void *)&d_long_rows};
    HIP_TRY(hipModuleLaunchKernel(m->fn_spmv_long, (unsigned)n_long, 1, 1, 256, 1, 1, 0, m->stream, largs, nullptr));
  }
  return IEM_OK;
}

/* ---- sharding (multi-GPU) ------------------------------------------------------------------- */
namespace {

void fill_shard_t(const iem::Model &M, const iem::ShardInfo &si, iem_shard_t *o) {
  std::memset(o, 0, sizeof *o);
  o->group = si.group; o->rank = si.rank; o->world = si.world; o->mailbox_kind = 0;
  o->n_global = si.n_global; o->own_lo = si.own_lo; o->own_n = si.own_n; o->halo = si.halo;
  o->halo_reach = si.halo_reach; o->halo_doubles = si.halo_doubles;
  o->nvar_global = si.nvar_global; o->ncon_global = si.ncon_global; o->nnzj_global = si.nnzj_global; o->nnzh_global = si.nnzh_global;
  o->nvar = M.nvar; o->ncon = M.ncon; o->nnzj = M.nnzj; o->nnzh = M.nnzh; o->n_templates = (int64_t)M.tpl.size();
  int64_t ns = 0;
  for (unsigned char f : si.var_flag) ns += (f & 2) ? 1 : 0;
  o->n_shared = ns;
}

void fill_shard_tpl(const iem::Model &M, const iem::ShardInfo &si, size_t i, iem_shard_template_t *o) {
  const iem::ShardTpl &st = si.tpl[i];
  const iem::Template &t = M.tpl[i];
  o->global_index = st.gindex; o->n_items = t.n_items;
  for (int d = 0; d < 3; ++d) { o->klo[d] = st.klo[d]; o->dims[d] = t.dims[d]; o->global_dims[d] = st.gdims[d]; }
  o->o0 = t.o0; o->o1 = t.o1; o->o2 = t.o2; o->global_o0 = st.go0; o->global_o1 = st.go1; o->global_o2 = st.go2;
  o->o1step = t.o1step; o->o2step = t.o2step; o->kind = t.kind;
  o->items_offset = -1;
  if (st.explicit_items) {
    int64_t off = 0;
    for (size_t j = 0; j < i; ++j) if (si.tpl[j].explicit_items) off += (int64_t)si.tpl[j].items.size();
    o->items_offset = off;
  }
}

std::vector<int64_t> shard_items(const iem::ShardInfo &si) {
  std::vector<int64_t> all;
  for (const iem::ShardTpl &st : si.tpl) if (st.explicit_items) all.insert(all.end(), st.items.begin(), st.items.end());
  return all;
}

// mailbox words: see iem_device.h
// the all-reduce runs on G workgroups, each on its own chunk of the NR doubles (one per 1 024, at most 64)
size_t mailbox_words(int64_t W, int64_t NH, int64_t NR, int64_t NL) {
  // header, reduce flags, halo data, reduce data, fold data; a two-sided shard: the second direction's block (8 words, halo data, fold data)
  return (size_t)(mailbox_b2(W, NH, NR) + (NL > 0 ? 8 + 4 * NL : 0));
}

struct CommHandle {   // what iem_comm_export writes (IEM_COMM_HANDLE_BYTES)
  hipIpcMemHandle_t ipc;
  int32_t pid, device, rank, world, kind, pad;
  int64_t words;
  uint64_t local_ptr;
  char bus[16];       // PCI bus id of the GPU the mailbox lives on ("0000:05:00.0"): device ordinals are per process
  uint64_t nonce;     // per-process random word: "same process" = same pid AND same nonce (pids repeat across PID namespaces)
};

uint64_t process_nonce() {
  static uint64_t n = 0;
  if (n == 0) {
    uint64_t v = 0;
    if (FILE *f = std::fopen("/dev/urandom", "rb")) { if (std::fread(&v, 8, 1, f) != 1) v = 0; std::fclose(f); }
    if (v == 0) v = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() * 0x9e3779b97f4a7c15ULL ^ ((uint64_t)getpid() << 32);
    n = v | 1;
  }
  return n;
}
static_assert(sizeof(CommHandle) <= IEM_COMM_HANDLE_BYTES, "comm handle too large");

}  // namespace

int iem_shard_blob(const void *blob, size_t nbytes, int group, int rank, int world, void **out_blob, size_t *out_nbytes,
                   iem_shard_t *out_info, int64_t **out_var_map, uint8_t **out_var_flag, iem_shard_template_t **out_tpl,
                   int64_t **out_items) {
  if (!blob || !out_blob || !out_nbytes) return fail(IEM_E_ARG, "null argument");
  try {
    iem::Model model;
    iem::ShardInfo si;
    iem::parse_blob(blob, nbytes, model);
    iem::shard_model(model, group, rank, world, si);
    std::vector<int64_t> w = iem::serialize_model(model);
    void *b = std::malloc(w.size() * 8);
    std::memcpy(b, w.data(), w.size() * 8);
    *out_blob = b; *out_nbytes = w.size() * 8;
    if (out_info) fill_shard_t(model, si, out_info);
    if (out_var_map) {
      *out_var_map = (int64_t *)std::malloc(sizeof(int64_t) * std::max<size_t>(si.var_map.size(), 1));
      if (!si.var_map.empty()) std::memcpy(*out_var_map, si.var_map.data(), si.var_map.size() * 8);
    }
    if (out_var_flag) {
      *out_var_flag = (uint8_t *)std::malloc(std::max<size_t>(si.var_flag.size(), 1));
      if (!si.var_flag.empty()) std::memcpy(*out_var_flag, si.var_flag.data(), si.var_flag.size());
    }
    if (out_tpl) {
      *out_tpl = (iem_shard_template_t *)std::malloc(sizeof(iem_shard_template_t) * std::max<size_t>(si.tpl.size(), 1));
      for (size_t i = 0; i < si.tpl.size(); ++i) fill_shard_tpl(model, si, i, *out_tpl + i);
    }
    if (out_items) {
      const std::vector<int64_t> all = shard_items(si);
      *out_items = (int64_t *)std::malloc(sizeof(int64_t) * std::max<size_t>(all.size(), 1));
      if (!all.empty()) std::memcpy(*out_items, all.data(), all.size() * 8);
    }
    return IEM_OK;
  } catch (const std::exception &e) {
    return fail(IEM_E_BLOB, e.what());
  }
}

int iem_shard_info(const iem_model *m, iem_shard_t *out) {
  if (!m || !out) return fail(IEM_E_ARG, "null argument");
  if (!m->sharded) return fail(IEM_E_ARG, "not a sharded handle (iem_create_sharded)");
  fill_shard_t(m->model, m->shard, out);
  out->mailbox_kind = m->mailbox_kind;
  return IEM_OK;
}

int iem_shard_halo(const iem_model *m, int64_t out[6]) {
  if (!m || !out) return fail(IEM_E_ARG, "null argument");
  if (!m->sharded) return fail(IEM_E_ARG, "not a sharded handle (iem_create_sharded)");
  const iem::ShardInfo &si = m->shard;
  out[0] = si.halo; out[1] = si.halo_right; out[2] = si.halo_reach; out[3] = si.reach_right;
  out[4] = si.halo_doubles; out[5] = si.halo_doubles_right;
  return IEM_OK;
}

int iem_shard_var_map(const iem_model *m, int64_t *h_map, uint8_t *h_flag) {
  if (!m) return fail(IEM_E_ARG, "null argument");
  if (!m->sharded) return fail(IEM_E_ARG, "not a sharded handle (iem_create_sharded)");
  if (h_map) std::memcpy(h_map, m->shard.var_map.data(), m->shard.var_map.size() * 8);
  if (h_flag) std::memcpy(h_flag, m->shard.var_flag.data(), m->shard.var_flag.size());
  return IEM_OK;
}

int iem_shard_template_info(const iem_model *m, int64_t i, iem_shard_template_t *out) {
  if (!m || !out) return fail(IEM_E_ARG, "null argument");
  if (!m->sharded) return fail(IEM_E_ARG, "not a sharded handle (iem_create_sharded)");
  if (i < 0 || i >= (int64_t)m->shard.tpl.size()) return fail(IEM_E_ARG, "bad template index");
  fill_shard_tpl(m->model, m->shard, (size_t)i, out);
  return IEM_OK;
}

int iem_shard_template_items(const iem_model *m, int64_t *h_items, int64_t *out_n) {
  if (!m || !out_n) return fail(IEM_E_ARG, "null argument");
  if (!m->sharded) return fail(IEM_E_ARG, "not a sharded handle (iem_create_sharded)");
  const std::vector<int64_t> all = shard_items(m->shard);
  *out_n = (int64_t)all.size();
  if (h_items && !all.empty()) std::memcpy(h_items, all.data(), all.size() * 8);
  return IEM_OK;
}

/* ---- mailboxes: halo exchange + the small all-reduce ------------------------------------------ */
int iem_comm_export(iem_model *m, void *out_handle) {
  if (!m || !out_handle) return fail(IEM_E_ARG, "null argument");
  if (!m->sharded) return fail(IEM_E_ARG, "not a sharded handle (iem_create_sharded)");
  DevGuard dg_(m->device);
  const iem::ShardInfo &si = m->shard;
  if (si.halo_reach > 0 || si.reach_right > 0)
    for (int r = 0; r < si.world; ++r) {   // a stencil must not reach past the neighbouring rank (either way)
      int64_t a, b;
      iem::partition_block(si.n_global, si.world, r, a, b);
      if (b - a < std::max(si.halo_reach, si.reach_right)) return fail(IEM_E_ARG, "a rank owns fewer supports than the stencil reaches");
    }
  int64_t ns = 0;
  for (unsigned char f : si.var_flag) ns += (f & 2) ? 1 : 0;
  m->n_shared = ns;
  m->mailbox_words = mailbox_words(si.world, si.halo_doubles, 1 + ns, si.halo_doubles_right);
  CommHandle h;
  std::memset(&h, 0, sizeof h);
  if (!m->mailbox) {
    // Peers write into this memory while a kernel here polls it: it must be FINE-GRAINED (coherent across
    // agents inside a kernel) — uncached device memory first, fine-grained next; plain hipMalloc memory is
    // the last resort (coherent only between processes sharing this GPU's L2: the one-GPU rehearsal) and
    // is reported through iem_shard_info().mailbox_kind so a multi-GPU host can refuse it.
    const unsigned flags[3] = {hipDeviceMallocUncached, hipDeviceMallocFinegrained, 0};
    for (int attempt = 0; attempt < 3 && !m->mailbox; ++attempt) {
      void *p = nullptr;
      hipError_t e = attempt < 2 ? hipExtMallocWithFlags(&p, m->mailbox_words * 8, flags[attempt]) : hipMalloc(&p, m->mailbox_words * 8);
      if (e != hipSuccess) { (void)hipGetLastError(); continue; }
      if (hipIpcGetMemHandle(&h.ipc, p) != hipSuccess) { (void)hipGetLastError(); hipFree(p); continue; }
      m->mailbox = (unsigned long long *)p;
      m->mailbox_kind = attempt == 0 ? 1 : attempt == 1 ? 3 : 2;
    }
    if (!m->mailbox) return fail(IEM_E_HIP, "could not allocate an IPC-exportable mailbox");
    HIP_TRY(hipMemset(m->mailbox, 0, m->mailbox_words * 8));
    HIP_TRY(hipDeviceSynchronize());
  } else {
    HIP_TRY(hipIpcGetMemHandle(&h.ipc, m->mailbox));
  }
  h.pid = (int32_t)getpid(); h.device = m->device; h.rank = si.rank; h.world = si.world; h.words = (int64_t)m->mailbox_words;
  h.kind = m->mailbox_kind;
  h.local_ptr = (uint64_t)(uintptr_t)m->mailbox;
  h.nonce = process_nonce();
  {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, m->device) != hipSuccess) { (void)hipGetLastError(); bus[0] = 0; }
    std::memcpy(h.bus, bus, sizeof(h.bus) - 1);   // h was zeroed: stays terminated
  }
  std::memset(out_handle, 0, IEM_COMM_HANDLE_BYTES);
  std::memcpy(out_handle, &h, sizeof h);
  return IEM_OK;
}

int iem_comm_connect(iem_model *m, const void *all_handles) {
  if (!m || !all_handles) return fail(IEM_E_ARG, "null argument");
  if (!m->sharded || !m->mailbox) return fail(IEM_E_ARG, "iem_comm_connect: call iem_comm_export on this handle first");
  if (m->connected) return fail(IEM_E_ARG, "already connected");
  DevGuard dg_(m->device);
  const iem::ShardInfo &si = m->shard;
  m->peers.assign((size_t)si.world, nullptr);
  CommHandle mine;
  std::memcpy(&mine, (const char *)all_handles + (size_t)si.rank * IEM_COMM_HANDLE_BYTES, sizeof mine);
  {
    // One process may drive several handles (one per GPU).  More than two on ONE device cannot work: their exchange
    // kernels spin on each other's flags and the streams of one process share hardware queues from the third on, so
    // a spinning kernel starves the peer it waits for (each call would end in the bounded time-out).  Refused here.
    int same = 0;
    for (int r = 0; r < si.world; ++r) {
      CommHandle h;
      std::memcpy(&h, (const char *)all_handles + (size_t)r * IEM_COMM_HANDLE_BYTES, sizeof h);
      if (h.pid == mine.pid && h.nonce == mine.nonce && std::strncmp(h.bus, mine.bus, sizeof h.bus) == 0) ++same;
    }
    if (same > 2)
      return fail(IEM_E_ARG, "iem_comm_connect: " + std::to_string(same) + " ranks of this communicator are handles of ONE process on ONE device; "
                             "at most two can exchange (one process per GPU is the supported form)");
  }
  for (int r = 0; r < si.world; ++r) {
    CommHandle h;
    std::memcpy(&h, (const char *)all_handles + (size_t)r * IEM_COMM_HANDLE_BYTES, sizeof h);
    if (h.rank != r || h.world != si.world || h.words != (int64_t)m->mailbox_words)
      return fail(IEM_E_ARG, "iem_comm_connect: handle " + std::to_string(r) + " does not belong to this communicator");
    // a kernel polls its mailbox while peers write into it: across GPUs that is only coherent for
    // fine-grained memory — refuse plain hipMalloc mailboxes there instead of timing out at run time
    if ((h.kind == 2 || mine.kind == 2) && std::strncmp(h.bus, mine.bus, sizeof h.bus) != 0)
      return fail(IEM_E_HIP, "iem_comm_connect: this runtime gave no fine-grained IPC memory for the mailboxes; "
                             "ranks on different GPUs cannot use them — fall back to the host's collective (RCCL) for obj/grad and copy the halo");
    if (r == si.rank) { m->peers[r] = m->mailbox; continue; }
    if (h.pid == (int32_t)getpid() && h.nonce == process_nonce()) {   // same process (one process driving several handles): the pointer itself
      if ((int)h.device != m->device) {
        hipError_t e = hipDeviceEnablePeerAccess((int)h.device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(IEM_E_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
        (void)hipGetLastError();
      }
      m->peers[r] = (unsigned long long *)(uintptr_t)h.local_ptr;
      continue;
    }
    void *p = nullptr;
    HIP_TRY(hipIpcOpenMemHandle(&p, h.ipc, hipIpcMemLazyEnablePeerAccess));
    m->ipc_opened.push_back(p);
    m->peers[r] = (unsigned long long *)p;
  }
  HIP_TRY(hipMalloc((void **)&m->d_peers, sizeof(void *) * (size_t)si.world));
  HIP_TRY(hipMemcpy(m->d_peers, m->peers.data(), sizeof(void *) * (size_t)si.world, hipMemcpyHostToDevice));
  // halo positions: what goes to the right neighbour (my last `reach` owned supports of every sharded
  // slab), where the left neighbour's arrive (my first `reach` window entries) — one canonical order
  // The second direction likewise: my FIRST `reach_right` owned supports go left, the right neighbour's arrive in my back
  // halo entries.  A rank at an end of the chain has no such entries: its positions are never used and stay 0.
  std::vector<long long> src, dst, src_l, dst_r;
  const int64_t own_end = si.halo + si.own_n;   // window coordinate behind the last owned support
  for (const iem::HaloSeg &sg : si.segs)
    for (int64_t o = 0; o < sg.outer; ++o) {
      const int64_t base = sg.loff + o * sg.wn * sg.inner;
      for (int64_t j = 0; j < si.halo_reach * sg.inner; ++j) {
        src.push_back(base + (own_end - si.halo_reach) * sg.inner + j);
        dst.push_back(base + j);
      }
      for (int64_t j = 0; j < si.reach_right * sg.inner; ++j) {
        src_l.push_back(base + si.halo * sg.inner + j);
        dst_r.push_back(si.halo_right == si.reach_right ? base + own_end * sg.inner + j : 0);
      }
    }
  if ((int64_t)src.size() != si.halo_doubles || (int64_t)src_l.size() != si.halo_doubles_right) return fail(IEM_E_ARG, "internal: halo size mismatch");
  if (!src_l.empty()) {
    HIP_TRY(hipMalloc((void **)&m->d_halo_src_l, src_l.size() * 8));
    HIP_TRY(hipMalloc((void **)&m->d_halo_dst_r, dst_r.size() * 8));
    HIP_TRY(hipMemcpy(m->d_halo_src_l, src_l.data(), src_l.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_halo_dst_r, dst_r.data(), dst_r.size() * 8, hipMemcpyHostToDevice));
  }
  if (!src.empty()) {
    HIP_TRY(hipMalloc((void **)&m->d_halo_src, src.size() * 8));
    HIP_TRY(hipMalloc((void **)&m->d_halo_dst, dst.size() * 8));
    HIP_TRY(hipMemcpy(m->d_halo_src, src.data(), src.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_halo_dst, dst.data(), dst.size() * 8, hipMemcpyHostToDevice));
  }
  std::vector<long long> sh;
  for (size_t i = 0; i < si.var_flag.size(); ++i) if (si.var_flag[i] & 2) sh.push_back((long long)i);
  if (!sh.empty()) {
    HIP_TRY(hipMalloc((void **)&m->d_shared, sh.size() * 8));
    HIP_TRY(hipMemcpy(m->d_shared, sh.data(), sh.size() * 8, hipMemcpyHostToDevice));
  }
  {
    HaloArgsH A = halo_args(m, nullptr);
    HIP_TRY(hipMalloc(&m->d_comm, sizeof A));
    HIP_TRY(hipMemcpy(m->d_comm, &A, sizeof A, hipMemcpyHostToDevice));
  }
  m->connected = true;
  return IEM_OK;
}

int iem_halo_exchange(iem_model *m, double *d_x) {
  if (!m || !d_x) return fail(IEM_E_ARG, "null argument");
  if (!m->connected) return fail(IEM_E_ARG, "iem_halo_exchange: not connected (iem_comm_connect)");
  const iem::ShardInfo &si = m->shard;
  if ((si.halo_doubles == 0 && si.halo_doubles_right == 0) || si.world == 1) return IEM_OK;   // no stencil crosses the shard boundary
  DevGuard dg_(m->device);
  int rc = halo_flush(m);   // one exchange at a time (the mailbox has two parity slots)
  if (rc) return rc;
  return halo_launch(m, d_x, m->stream);
}

int iem_halo_exchange_async(iem_model *m, double *d_x) {
  if (!m || !d_x) return fail(IEM_E_ARG, "null argument");
  if (!m->connected) return fail(IEM_E_ARG, "iem_halo_exchange_async: not connected (iem_comm_connect)");
  const iem::ShardInfo &si = m->shard;
  if ((si.halo_doubles == 0 && si.halo_doubles_right == 0) || si.world == 1) return IEM_OK;
  DevGuard dg_(m->device);
  int rc = halo_flush(m);   // an earlier exchange nobody carried: it goes first, in order
  if (rc) return rc;
  m->halo_deferred = true;
  m->halo_vec = d_x;
  return IEM_OK;
}

int iem_halo_wait(iem_model *m) {
  if (!m) return fail(IEM_E_ARG, "null handle");
  DevGuard dg_(m->device);
  return halo_flush(m);
}

int iem_halo_reads(const iem_model *m, int kind, int *out_x, int *out_v, int *out_carrier) {
  if (!m || kind < 0 || kind > iem::KK_LAST) return fail(IEM_E_ARG, "bad argument");
  if (out_x) *out_x = m->reads_halo_x[kind] ? 1 : 0;
  if (out_v) *out_v = m->reads_halo_v[kind] ? 1 : 0;
  if (out_carrier) *out_carrier = (m->carrier[kind] && !m->reads_halo_x[kind]) ? 1 : 0;
  return IEM_OK;
}

int iem_halo_fold(iem_model *m, double *d_vec) {
  if (!m || !d_vec) return fail(IEM_E_ARG, "null argument");
  if (!m->connected) return fail(IEM_E_ARG, "iem_halo_fold: not connected (iem_comm_connect)");
  const iem::ShardInfo &si = m->shard;
  if ((si.halo_doubles == 0 && si.halo_doubles_right == 0) || si.world == 1) return IEM_OK;
  DevGuard dg_(m->device);
  { int rc = halo_flush(m); if (rc) return rc; }
  // IemFoldArgs, and behind it what IemFold2Args adds (iem_halo2_device.h)
  struct { double *vec; unsigned long long *mine, *left, *right; const long long *src, *dst; long long NH, W, G, NR; unsigned long long *hstatus; long long ticks;
           const long long *src_l, *dst_r; long long NL, B2; } A = {
      d_vec, m->mailbox, si.rank > 0 ? m->peers[si.rank - 1] : nullptr, si.rank + 1 < si.world ? m->peers[si.rank + 1] : nullptr,
      m->d_halo_src, m->d_halo_dst, (long long)si.halo_doubles, (long long)si.world, (long long)reduce_chunks(1 + m->n_shared),
      (long long)(1 + m->n_shared), m->d_hstatus, (long long)m->opt.comm_timeout_ms * 100000LL,
      m->d_halo_src_l, m->d_halo_dst_r, (long long)si.halo_doubles_right, (long long)mailbox_b2(si.world, si.halo_doubles, 1 + m->n_shared)};
  return launch_args(m->fn_fold, &A, m->opt.two_sided ? sizeof A : 12 * 8, 1, 1, 256, 0, m->stream);
}

int iem_allreduce_obj_grad(iem_model *m, double *d_obj, double *d_g) {
  if (!m) return fail(IEM_E_ARG, "null argument");
  if (!m->connected) return fail(IEM_E_ARG, "iem_allreduce_obj_grad: not connected (iem_comm_connect)");
  if (!d_g && m->n_shared) return fail(IEM_E_ARG, "null gradient but the model has replicated variables");
  DevGuard dg_(m->device);
  // Every rank must issue its mailbox kernels in the SAME order.  Whether an evaluation call in between flushed a deferred
  // exchange depends on the rank (rank 0 holds no halo copies: its reads_halo is false), so a collective never overtakes a
  // deferred exchange: it goes first, as in iem_halo_fold / iem_comm_status / iem_synchronize.
  { int rc = halo_flush(m); if (rc) return rc; }
  const iem::ShardInfo &si = m->shard;
  const long long G = (long long)reduce_chunks(1 + m->n_shared);
  struct { double *obj, *g; const long long *shared; unsigned long long *const *peers; long long NR, NH, W, rank, G; unsigned long long *hstatus; long long ticks; } A = {
      d_obj, d_g, m->d_shared, m->d_peers, (long long)(1 + m->n_shared), (long long)si.halo_doubles, (long long)si.world, (long long)si.rank, G,
      m->d_hstatus, (long long)m->opt.comm_timeout_ms * 100000LL};
  return launch_args(m->fn_reduce, &A, sizeof A, (unsigned)G, 1, 256, 0, m->stream);
}

int iem_comm_status(iem_model *m, int64_t *out_status) {
  if (!m || !out_status) return fail(IEM_E_ARG, "null argument");
  if (!m->mailbox) return fail(IEM_E_ARG, "no mailbox");
  DevGuard dg_(m->device);
  { int rc = halo_flush(m); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(m->stream));
  unsigned long long st = 0;
  HIP_TRY(hipMemcpy(&st, m->mailbox, 8, hipMemcpyDeviceToHost));
  *out_status = (int64_t)st;
  return IEM_OK;
}

/* ---- chain KKT solver ------------------------------------------------------------------------------ */
namespace {
// Shape of a kkt_eliminate workgroup: waves (KKT_WMAX of csrc/iem_kkt_device.h; a wave owns every KKT_WMAX-th 16-row tile row)
// and the register budget as waves per SIMD (KKT_WPE).  The block inverse is a chain of dependent panel steps, each of which
// reads the whole row panel from LDS IN EVERY WAVE: few waves with many tiles each — and many workgroups per CU to hide the
// chain's latency — beat one wave per tile row (quadrotor_oc3, 84 x 84 blocks: 11.6 ms with four waves, 10.3 with six, 5.8
// with two; 40 x 40: 2.60 -> 2.40 with one).  With a border the products Z = D^-1 E and E' Z dominate and want the waves
// (OPF, 60 + 52: 3.6 ms with four, 4.6 with two, 7.0 with one).  profiles/r03_kkt_shape_ab.txt
struct KktKnobs { int wmax = -1, wpe = -1, rowwise = -1, wpg = -1; std::string contract = "off", defs; };
KktKnobs kkt_knobs() {
  KktKnobs k;
  const char *on = getenv("IEM_KKT_EXPERIMENTS");
  if (!on || std::strcmp(on, "1") != 0) return k;     // production: the environment cannot change kernel shape, numerics or source
  if (const char *e = getenv("IEM_KKT_WMAX")) { const int v = atoi(e); if (v >= 1 && v <= 6) k.wmax = v; }
  if (const char *e = getenv("IEM_KKT_WPE")) { const int v = atoi(e); if (v >= 0 && v <= 8) k.wpe = v; }
  if (const char *e = getenv("IEM_KKT_WPG")) { const int v = atoi(e); if (v == 1 || v == 2) k.wpg = v; }
  if (const char *e = getenv("IEM_KKT_ROWWISE")) { const int v = atoi(e); if (v >= 0 && v <= 2) k.rowwise = v; }
  if (const char *e = getenv("IEM_KKT_CONTRACT")) { if (!std::strcmp(e, "fast") || !std::strcmp(e, "on") || !std::strcmp(e, "off")) k.contract = e; }
  if (const char *e = getenv("IEM_KKT_DEFS")) {        // extra "#define NAME VALUE" lines only: [A-Za-z0-9_ #\n]
    bool ok = true;
    for (const char *c = e; *c; ++c) ok = ok && (std::isalnum((unsigned char)*c) || *c == '_' || *c == ' ' || *c == '#' || *c == '\n');
    if (ok) k.defs = e;
  }
  return k;
}
// kkt_eliminate's other form (KKT_ROWWISE of csrc/iem_kkt_device.h): lane = row, 64 / nb blocks per one-wave workgroup — blocks
// without a border that fit the lanes of a wave
// ... returns the rows a lane holds (KKT_RPL): 0 = the matrix-core panel form
int kkt_rowwise(int nb, int ne) {
  static const KktKnobs knobs = kkt_knobs();
  if (ne != 0 || nb > 48) return 0;
  if (knobs.rowwise >= 0) return knobs.rowwise;
  // two rows per lane up to 24 x 24 (hovercraft 20 x 20 at 1e5 supports: 0.74 ms against 0.84 with one row and 1.66 in the panel form); one
  // row up to 40 (40 x 40: 1.96 ms against 2.40 in the panel form, three blocks per two-wave workgroup — kkt_row_wpg; two rows of 40 leave one
  // wave per SIMD: 2.9 ms; 44 x 44 spills: 7.3 ms);
  // beyond that the panel form.  profiles/r04_kkt_rpl_ab.txt
  return nb <= 24 ? 2 : nb <= 40 ? 1 : 0;
}
// ne = -1: no border and ONE block per launch (the pivot blocks of the hubs' dense LDL', one after the other): nothing hides the
// block's own latency, so every tile row gets a wave (96 x 96: 50 -> 38 us per block; profiles/r04_kkt_leaf_shape_ab.txt)
// waves per workgroup of the lane-per-row eliminate: two when that fills the lanes better (40 lanes per block: 3 blocks on 128 lanes
// instead of 1 on 64 — the kernel is bound by the LDS reads every lane of the workgroup makes, idle or not)
int kkt_row_wpg(int nb, int ne) {
  static const KktKnobs knobs = kkt_knobs();
  const int rpl = kkt_rowwise(nb, ne);
  if (!rpl) return 1;
  if (knobs.wpg >= 1) return knobs.wpg;
  const int lpb = nb / rpl;
  return (128 / lpb) * 64 > (64 / lpb) * 128 ? 2 : 1;      // blocks per lane, two waves against one
}
void kkt_shape(int nb, int ne, int *wmax, int *wpe) {
  const int R = (nb + 15) / 16;
  if (ne < 0) { *wmax = 6; *wpe = 0; return; }
  if (ne > 0 || R <= 2) { *wmax = 4; *wpe = nb <= 48 ? 4 : 0; }
  else if (R == 3) { *wmax = 1; *wpe = 3; }
  else if (R == 4) { *wmax = 2; *wpe = 3; }
  else { *wmax = 2; *wpe = 2; }
  // experiment overrides (tools/sessions/kkt_shape_ab.sh): honoured only when IEM_KKT_EXPERIMENTS=1, and read ONCE per process —
  // the launch shape of a cached module can never drift from the KKT_T it was compiled with
  static const KktKnobs knobs = kkt_knobs();
  if (knobs.wmax >= 1) *wmax = knobs.wmax;
  if (knobs.wpe >= 0) *wpe = knobs.wpe;
}
// Columns per chunk of the multi-column solves (KKT_MR of csrc/iem_kkt_many_device.h).  Four, from the measurement and the
// register use together (profiles/kkt_solve_many.json): at four every multi-column kernel of the precompiled shapes stays
// within 184 VGPRs (<= 138 up to 52 x 52 blocks: three to four waves per SIMD) and a column costs half a single solve; eight
// takes kkt_forward_m / kkt_fs_m to 216 - 256 VGPRs (two waves) for another 3 - 15 % per column at nrhs >= 8 and LOSES 4 - 31 %
// at nrhs = 4 (a half-empty chunk).  Two where kkt_fs_m's per-lane state (MR x nc doubles of z) would be wide.
int kkt_many_width(int nb, int ne, int nc) { return (kkt_rowwise(nb, ne) && nb <= 32 && nc > 16) ? 2 : 4; }
std::string kkt_source(int nb, int ne, int nc) {
  // (fused multiply-adds would be allowed here — nothing compares these kernels bit for bit — and take 1 000 of the 2 350 FP64
  // instructions out of a 40 x 40 kkt_eliminate, but the factorisation does not get faster for it: 2.52 against 2.45 ms at 1e5
  // quadrotor supports, 3.22 against 3.54 for the bordered OPF blocks, solves 9 % slower — the panel steps wait on their
  // dependency chain, not on issue slots.  IEM_KKT_CONTRACT=fast switches them on; profiles/r03_kkt_shape_ab.txt)
  static const KktKnobs knobs = kkt_knobs();
  std::string s = source_prelude(knobs.contract);
  s += "#define KKT_NB " + std::to_string(nb) + "\n#define KKT_NE " + std::to_string(std::max(ne, 0)) + "\n#define KKT_NC " + std::to_string(nc) + "\n";
  int wmax, wpe;
  kkt_shape(nb, ne, &wmax, &wpe);
  if (wpe > 0) s += "#define KKT_WPE " + std::to_string(wpe) + "\n";
  if (wmax != 4) s += "#define KKT_WMAX " + std::to_string(wmax) + "\n";
  if (kkt_rowwise(nb, ne)) s += "#define KKT_ROWWISE " + std::to_string(kkt_rowwise(nb, ne)) + "\n#define KKT_ROW_WPG " + std::to_string(kkt_row_wpg(nb, ne)) + "\n";
  if (!knobs.defs.empty()) s += knobs.defs + "\n";     // (experiments, IEM_KKT_EXPERIMENTS=1 only: extra #define lines)
  s += "#define KKT_MR " + std::to_string(kkt_many_width(nb, ne, nc)) + "\n";
  s += kKktSource;
  s += kKktManySource;
  return s;
}
// LDS the kernels of a shape DECLARE, from the quantities of csrc/iem_kkt_device.h.  kkt_eliminate, lane-per-row form: two pivot-row
// buffers of KKT_BPW blocks and the two counters; panel form: the column and row panels of the inverse (two of each, 16 R rows of stride
// KKT_LC = 5 and 4 rows of stride KKT_LP = 16 R + 1, R = ceil(nb / 16) tile rows — NOT nb: the rim is part of the buffers), the 2 x 32
// doubles of the pivot blocks and the two counters, and with a border one NB x NB and two NB x NE tiles (strides nb + 1, ne + 1).
// kkt_update: seven NC x NC tiles (and the two index tables, within the allowance).
long long kkt_lds_eliminate(int nb, int ne) {
  if (const int rpl = kkt_rowwise(nb, ne)) return 16LL * ((64 * kkt_row_wpg(nb, ne)) / (nb / rpl)) * nb + 8;
  const long long R = (nb + 15) / 16;
  return 8LL * (2 * 16 * R * 5 + 2 * 4 * (16 * R + 1) + 64) + 8 + (ne > 0 ? 8LL * nb * (nb + 1) + 16LL * nb * (ne + 1) : 0);
}
bool kkt_fits(int nb, int ne, int nc) {
  const long long upd = 56LL * nc * (nc + 1) + 1024;
  return kkt_lds_eliminate(nb, ne) <= 160 * 1024 && upd <= 160 * 1024;
}
// The shapes a chain KKT code object exists for: what iem_kkt_source emits and kkt_module loads — one rule, one message
int kkt_admit(int nb, int ne, int nc) {
  if (nb < 4 || nb > 96 || nb % 4 || ne < -1 || ne > 128 || (ne > 0 && ne % 4) || nc < 4 || nc > 48 || nc % 4 || nc > nb || !kkt_fits(nb, ne, nc))
    return fail(IEM_E_ARG, "chain KKT: block size must be a multiple of 4 in 4..96, border size a multiple of 4 in 0..128, coupling width a multiple of 4 in 4..48 (and <= the block size), tiles within the LDS of a CU");
  return IEM_OK;
}
// The kernels of a chain KKT code object and where kkt_module keeps them.  `lane_rows_only`: the lane-per-row solves (csrc/iem_kkt_device.h:
// kkt_fz / kkt_fs / kkt_bw, and their multi-column forms), resolved only for the shapes whose eliminate is lane-per-row too and nb <= 32:
// at 40 x 40 they lose 12 % to the 64-thread kernels (two launches per level, 40 of 64 lanes), at 20 x 20 they win 30 %
typedef iem_model::KktMod KM;
const struct KktSlot { const char *name; hipFunction_t KM::*fn; bool lane_rows_only; } kKktSlots[] = {
    {"kkt_eliminate", &KM::elim, false}, {"kkt_update", &KM::upd, false}, {"kkt_forward", &KM::fwd, false}, {"kkt_backward", &KM::bwd, false},
    {"kkt_hub_z", &KM::hub_z, false}, {"kkt_hub_widen", &KM::hub_widen, false}, {"kkt_hub_mask", &KM::hub_mask, false}, {"kkt_hub_ety", &KM::hub_ety, false},
    {"kkt_hub_ex", &KM::hub_ex, false}, {"kkt_hub_leaf", &KM::hub_leaf, false}, {"kkt_hub_diagmax", &KM::hub_diagmax, false},
    {"kkt_fz", &KM::fz, true}, {"kkt_fs", &KM::fs, true}, {"kkt_bw", &KM::bw, true}, {"kkt_fz_m", &KM::fz_m, true}, {"kkt_fs_m", &KM::fs_m, true}, {"kkt_bw_m", &KM::bw_m, true},
    {"kkt_forward_m", &KM::fwd_m, false}, {"kkt_backward_m", &KM::bwd_m, false}, {"kkt_move_m", &KM::move_m, false}, {"kkt_colsum_m", &KM::colsum_m, false},
};
int kkt_module(iem_model *m, int nb, int ne, int nc, iem_model::KktMod **out) {
  if (int rc = kkt_admit(nb, ne, nc)) return rc;
  auto it = m->kkt_mods.find({nb, ne * 64 + nc});
  if (it == m->kkt_mods.end()) {
    iem_model::KktMod km;
    const bool lane_rows = kkt_rowwise(nb, ne) && nb <= 32;
    KernelSlot slots[sizeof kKktSlots / sizeof *kKktSlots];
    int n = 0;
    for (const KktSlot &ks : kKktSlots)
      if (lane_rows || !ks.lane_rows_only) slots[n++] = KernelSlot{ks.name, &(km.*ks.fn)};
    int rc = load_object(m, kkt_source(nb, ne, nc), slots, n, &km.mod);
    if (rc) return rc;
    int wmax, wpe_;
    kkt_shape(nb, ne, &wmax, &wpe_);
    km.elim_wg = 64u * (unsigned)std::min((nb + 15) / 16, wmax);   // KKT_T of csrc/iem_kkt_device.h
    if (kkt_rowwise(nb, ne)) { km.elim_wg = 64u * (unsigned)kkt_row_wpg(nb, ne); km.elim_bpw = (int)km.elim_wg / (nb / kkt_rowwise(nb, ne)); }
    if (lane_rows) km.solve_bpw = 64 / nb;
    km.many_r = kkt_many_width(nb, ne, nc);
    it = m->kkt_mods.emplace(std::make_pair(nb, ne * 64 + nc), km).first;
  }
  *out = &it->second;
  return IEM_OK;
}
struct KktArgsH { double *D, *Bt, *BR, *E, *Z, *Gp; const int *rows, *cols; long long *info; long long S, s; int final_block; double tiny; long long T = 0; };
struct KktSolveArgsH { const double *D, *Bt, *BR, *Z; const int *rows, *cols; double *r, *z, *rBp; const double *xB; long long S, s; int final_block; long long T = 0; };
// (an empty grid launches nothing; `cols`: the grid's second extent)
int kkt_launch_raw(iem_model *m, hipFunction_t fn, void *args, size_t sz, long long grid, unsigned block, int cols = 1) {
  if (grid <= 0 || cols <= 0) return IEM_OK;
  return launch_args(fn, args, sz, (unsigned)grid, (unsigned)cols, block, 0, m->stream);
}
int kkt_launch(iem_model *m, hipFunction_t fn, KktArgsH a, long long grid, unsigned block) { return kkt_launch_raw(m, fn, &a, sizeof a, grid, block); }
int kkt_launch_solve(iem_model *m, hipFunction_t fn, KktSolveArgsH a, long long grid, unsigned block) { return kkt_launch_raw(m, fn, &a, sizeof a, grid, block); }
struct KktSolveManyArgsH { KktSolveArgsH a; int nr; };      // KktSolveManyArgs of csrc/iem_kkt_many_device.h
int kkt_launch_many(iem_model *m, hipFunction_t fn, const KktSolveArgsH &a, int nr, long long grid, unsigned block) {
  KktSolveManyArgsH A{a, nr};
  return kkt_launch_raw(m, fn, &A, sizeof A, grid, block);
}
// (experiments only: the 64-thread solves for every shape)
bool kkt_old_solves() {
  static const bool v = [] { const char *e = getenv("IEM_KKT_EXPERIMENTS"), *o = getenv("IEM_KKT_OLD_SOLVES"); return e && !std::strcmp(e, "1") && o && !std::strcmp(o, "1"); }();
  return v;
}
// kkt_eliminate over `blocks` blocks of the level: a workgroup takes elim_bpw of them
int kkt_launch_elim(iem_model *m, const iem_model::KktMod *km, KktArgsH a, long long blocks) {
  return kkt_launch_raw(m, km->elim, &a, sizeof a, (blocks + km->elim_bpw - 1) / km->elim_bpw, km->elim_wg);
}
}  // namespace

int iem_kkt_source(int nb, int ne, int nc, char **out_src, uint64_t *out_key) {
  if (int rc = kkt_admit(nb, ne, nc)) return rc;      // (what no handle would load has no source either: the CPU can sweep admission)
  return emit_out(kkt_source(nb, ne, nc), out_src, out_key);
}

int iem_kkt_chain_factor(iem_model *m, int64_t S, int nb, int ne, int nc, double *d_D, double *d_Bt, double *d_BR, const int32_t *d_rows,
                         const int32_t *d_cols, double *d_E, double *d_Z, double *d_Gp, int64_t *d_info, double tiny) {
  const bool chained = d_Bt != nullptr;   // d_Bt == NULL: the blocks do not couple to each other (reach 0), only to the border
  if (!m || S < 1 || !d_D || (chained && (!d_BR || !d_rows || !d_cols)) || !d_info || (ne > 0 && (!d_E || !d_Z || !d_Gp))) return fail(IEM_E_ARG, "bad argument");
  DevGuard dg_(m->device);
  iem_model::KktMod *km = nullptr;
  int rc = kkt_module(m, nb, ne, nc, &km);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(d_info, 0, 24, m->stream));
  KktArgsH A{d_D, d_Bt, d_BR, d_E, d_Z, d_Gp, d_rows, d_cols, (long long *)d_info, (long long)S, 1, 0, tiny};
  if (!chained) {   // one launch: every block against the border
    A.final_block = 2;
    return kkt_launch_elim(m, km, A, S);
  }
  for (long long s = 1; s < S; s *= 2) {   // level: eliminate the odd multiples of s, fold them into the even ones
    A.s = s;
    const long long n_elim = (S - s + 2 * s - 1) / (2 * s), n_surv = (S + 2 * s - 1) / (2 * s);
    if ((rc = kkt_launch_elim(m, km, A, n_elim)) != IEM_OK) return rc;
    if ((rc = kkt_launch(m, km->upd, A, n_surv, nc <= 8 ? 64u : nc <= 16 ? 128u : 256u)) != IEM_OK) return rc;   // KKT_TU
  }
  A.final_block = 1;
  return kkt_launch_elim(m, km, A, 1);
}

/* ONE step of the same reduction, for a caller that interleaves work of its own between the levels (kkt_chain.HubChainKKT: the
 * span-sparse border of a laned 2-D grid).  what = 0: eliminate the blocks (2t+1)s (in-place inverses, BR kept), 1: fold them
 * into the survivors 2ts, 2: the last remaining block (index 0), 3: clear the pivot counters.  No border (ne = 0 module). */
int iem_kkt_chain_level(iem_model *m, int64_t S, int64_t lane_len, int nb, int nc, double *d_D, double *d_Bt, double *d_BR, const int32_t *d_rows,
                        const int32_t *d_cols, int64_t *d_info, double tiny, int64_t s, int what) {
  const long long T = lane_len > 0 ? lane_len : S;
  if (!m || S < 1 || S % T || !d_D || !d_Bt || !d_BR || !d_rows || !d_cols || !d_info || s < 1 || what < 0 || what > 3) return fail(IEM_E_ARG, "bad argument");
  DevGuard dg_(m->device);
  if (what == 3) { HIP_TRY(hipMemsetAsync(d_info, 0, 24, m->stream)); return IEM_OK; }
  iem_model::KktMod *km = nullptr;
  int rc = kkt_module(m, nb, 0, nc, &km);
  if (rc) return rc;
  const long long lanes = S / T;
  KktArgsH A{d_D, d_Bt, d_BR, nullptr, nullptr, nullptr, d_rows, d_cols, (long long *)d_info, (long long)S, (long long)s, 0, tiny, T};
  if (what == 2) { A.final_block = 1; A.s = 1; return kkt_launch_elim(m, km, A, lanes); }
  if (s >= T) return IEM_OK;
  const long long n_elim = lanes * ((T - s + 2 * s - 1) / (2 * s)), n_surv = lanes * ((T + 2 * s - 1) / (2 * s));
  if (what == 0) return kkt_launch_elim(m, km, A, n_elim);
  return kkt_launch(m, km->upd, A, n_surv, nc <= 8 ? 64u : nc <= 16 ? 128u : 256u);
}

/* The span-sparse border columns of HubChainKKT between two levels (csrc/iem_kkt_device.h: kkt_hub_z, kkt_hub_widen). */
int iem_kkt_hub_level(iem_model *m, int64_t S, int64_t lane_len, int nb, int nc, const double *d_Dinv, const double *d_Bt, const int32_t *d_q, int nq,
                      const int32_t *d_qr, int nr, const int32_t *d_qc, int ncq, int hw, int64_t s, const double *d_E, double *d_Z, double *d_En, int last) {
  const long long T = lane_len > 0 ? lane_len : S;
  if (!m || S < 1 || S % T || !d_Dinv || !d_Bt || !d_q || !d_qr || !d_qc || nq < 1 || nq > 24 || nr < 0 || ncq < 0 || nr > nc || ncq > nc || hw < 1 || s < 1 || !d_E || !d_Z ||
      (!last && (!d_En || s >= T)))
    return fail(IEM_E_ARG, "bad argument");
  DevGuard dg_(m->device);
  iem_model::KktMod *km = nullptr;
  int rc = kkt_module(m, nb, 0, nc, &km);
  if (rc) return rc;
  struct { const double *D, *Bt, *E, *Z; double *out; const int *q, *qr, *qc; long long T, lanes, s, n_e, n_s; int nb, nc, nq, nr, ncq, hw, last; } A{
      d_Dinv, d_Bt, d_E, nullptr, d_Z, d_q, d_qr, d_qc, T, S / T, (long long)s, 0, 0, nb, nc, nq, nr, ncq, hw, last ? 1 : 0};
  const long long alive = (T + s - 1) / s, W = (2 * s - 1) * hw, W2 = (4 * s - 1) * hw;
  A.n_e = alive / 2; A.n_s = alive - A.n_e;
  const long long nz = (last ? 1 : A.n_e) * A.lanes * W;
  if ((rc = kkt_launch_raw(m, km->hub_z, &A, sizeof A, (nz + 255) / 256, 256)) != IEM_OK || last) return rc;
  A.Z = d_Z; A.out = d_En;
  return kkt_launch_raw(m, km->hub_widen, &A, sizeof A, (A.n_s * A.lanes * W2 + 255) / 256, 256);
}

int iem_kkt_chain_solve(iem_model *m, int64_t S, int nb, int ne, int nc, const double *d_Dinv, const double *d_Bt, const double *d_BR,
                        const int32_t *d_rows, const int32_t *d_cols, const double *d_Z, double *d_r, double *d_z, double *d_rBp,
                        const double *d_xB, int phase) {
  return iem_kkt_chain_solve_lanes(m, S, S, nb, ne, nc, d_Dinv, d_Bt, d_BR, d_rows, d_cols, d_Z, d_r, d_z, d_rBp, d_xB, phase);
}

int iem_kkt_chain_solve_lanes(iem_model *m, int64_t S, int64_t lane_len, int nb, int ne, int nc, const double *d_Dinv, const double *d_Bt, const double *d_BR,
                              const int32_t *d_rows, const int32_t *d_cols, const double *d_Z, double *d_r, double *d_z, double *d_rBp,
                              const double *d_xB, int phase) {
  const bool chained = d_Bt != nullptr;   // as in iem_kkt_chain_factor
  const long long T = lane_len > 0 ? lane_len : S;
  if (!m || S < 1 || S % T || (T != S && ne > 0) || !d_Dinv || (chained && (!d_BR || !d_rows || !d_cols || !d_z)) || !d_r || (ne > 0 && (!d_Z || (phase == 0 && !d_rBp) || (phase == 1 && !d_xB)))) return fail(IEM_E_ARG, "bad argument");
  DevGuard dg_(m->device);
  iem_model::KktMod *km = nullptr;
  int rc = kkt_module(m, nb, ne, nc, &km);
  if (rc) return rc;
  const long long lanes = S / T;
  KktSolveArgsH A{d_Dinv, d_Bt, d_BR, d_Z, d_rows, d_cols, d_r, d_z, d_rBp, d_xB, (long long)S, 1, 0, T};
  const bool rowwise = km->fz && !kkt_old_solves();        // no border, blocks that fit a wave: a lane per row
  const long long bpw = rowwise ? km->solve_bpw : 1;
  if (!chained) {            // independent blocks: the border terms of all blocks (forward), every block's own solve (backward)
    if (phase != 0 && phase != 1) return fail(IEM_E_ARG, "phase must be 0 (forward) or 1 (backward)");
    A.final_block = 2;
    if (phase == 0) return ne > 0 ? kkt_launch_solve(m, km->fwd, A, S, 64) : IEM_OK;
    return rowwise ? kkt_launch_solve(m, km->fz, A, (S + bpw - 1) / bpw, 64) : kkt_launch_solve(m, km->bwd, A, S, 64);
  }
  if (phase == 0 && rowwise) {
    for (long long s = 1; s < T; s *= 2) {
      A.s = s;
      const long long n_elim = lanes * ((T - s + 2 * s - 1) / (2 * s)), n_surv = lanes * ((T + 2 * s - 1) / (2 * s));
      if ((rc = kkt_launch_solve(m, km->fz, A, (n_elim + bpw - 1) / bpw, 64)) != IEM_OK) return rc;      // z of the level's eliminated blocks ...
      if ((rc = kkt_launch_solve(m, km->fs, A, (n_surv + 63) / 64, 64)) != IEM_OK) return rc;            // ... folded into the survivors' right-hand sides
    }
    return IEM_OK;
  }
  if (phase == 0) {          // forward: levels up, then the last block's border contribution
    for (long long s = 1; s < T; s *= 2) {
      A.s = s;
      const long long n_elim = lanes * ((T - s + 2 * s - 1) / (2 * s)), n_surv = lanes * ((T + 2 * s - 1) / (2 * s));
      if ((rc = kkt_launch_solve(m, km->fwd, A, n_surv + n_elim, 64)) != IEM_OK) return rc;
    }
    A.final_block = 1;
    return ne > 0 ? kkt_launch_solve(m, km->fwd, A, lanes, 64) : IEM_OK;
  }
  if (phase != 1) return fail(IEM_E_ARG, "phase must be 0 (forward) or 1 (backward)");
  A.final_block = 1;
  if ((rc = rowwise ? kkt_launch_solve(m, km->fz, A, (lanes + bpw - 1) / bpw, 64) : kkt_launch_solve(m, km->bwd, A, lanes, 64)) != IEM_OK) return rc;
  A.final_block = 0;
  long long top = 1;
  while (top * 2 < T) top *= 2;
  for (long long s = top; s >= 1; s /= 2) {
    if (s >= T) continue;
    A.s = s;
    const long long n_elim = lanes * ((T - s + 2 * s - 1) / (2 * s));
    if ((rc = rowwise ? kkt_launch_solve(m, km->bw, A, (n_elim + bpw - 1) / bpw, 64) : kkt_launch_solve(m, km->bwd, A, n_elim, 64)) != IEM_OK) return rc;
  }
  return IEM_OK;
}

/* The same levels for nrhs right-hand sides (csrc/iem_kkt_many_device.h): column u of r / z is the plane d_r + u S nb, of rBp
 * d_rBp + u S ne, of xB d_xB + u ne.  Chunks of the shape's width (kkt_many_width) share every read of the factors; a chunk of
 * ONE column goes through the single-column kernels — whose operations, per column, the multi-column kernels repeat in the
 * same order: a column's bits do not depend on how the columns were chunked. */
int iem_kkt_chain_solve_many(iem_model *m, int64_t S, int64_t lane_len, int nb, int ne, int nc, const double *d_Dinv, const double *d_Bt, const double *d_BR,
                             const int32_t *d_rows, const int32_t *d_cols, const double *d_Z, double *d_r, double *d_z, double *d_rBp,
                             const double *d_xB, int nrhs, int phase) {
  const bool chained = d_Bt != nullptr;
  const long long T = lane_len > 0 ? lane_len : S;
  if (!m || nrhs < 1 || S < 1 || S % T || (T != S && ne > 0) || !d_Dinv || (chained && (!d_BR || !d_rows || !d_cols || !d_z)) || !d_r || (ne > 0 && (!d_Z || (phase == 0 && !d_rBp) || (phase == 1 && !d_xB))))
    return fail(IEM_E_ARG, "bad argument");
  if (phase != 0 && phase != 1) return fail(IEM_E_ARG, "phase must be 0 (forward) or 1 (backward)");
  DevGuard dg_(m->device);
  iem_model::KktMod *km = nullptr;
  int rc = kkt_module(m, nb, ne, nc, &km);
  if (rc) return rc;
  const long long lanes = S / T, nep = std::max(ne, 0);
  const bool rowwise = km->fz_m && !kkt_old_solves();
  const long long bpw = rowwise ? km->solve_bpw : 1;
  for (int c0 = 0; c0 < nrhs; c0 += km->many_r) {
    const int nr = std::min(km->many_r, nrhs - c0);
    double *r = d_r + (long long)c0 * S * nb, *z = d_z ? d_z + (long long)c0 * S * nb : nullptr, *rBp = d_rBp ? d_rBp + (long long)c0 * S * nep : nullptr;
    const double *xB = d_xB ? d_xB + (long long)c0 * nep : nullptr;
    if (nr == 1) {
      if ((rc = iem_kkt_chain_solve_lanes(m, S, lane_len, nb, ne, nc, d_Dinv, d_Bt, d_BR, d_rows, d_cols, d_Z, r, z, rBp, xB, phase))) return rc;
      continue;
    }
    KktSolveArgsH A{d_Dinv, d_Bt, d_BR, d_Z, d_rows, d_cols, r, z, rBp, xB, (long long)S, 1, 0, T};
    auto go = [&](hipFunction_t fn, long long grid) { return kkt_launch_many(m, fn, A, nr, grid, 64); };
    if (!chained) {            // independent blocks: the border terms of all blocks (forward), every block's own solve (backward)
      A.final_block = 2;
      if (phase == 0) rc = ne > 0 ? go(km->fwd_m, S) : IEM_OK;
      else rc = rowwise ? go(km->fz_m, (S + bpw - 1) / bpw) : go(km->bwd_m, S);
      if (rc) return rc;
      continue;
    }
    if (phase == 0) {
      for (long long s = 1; s < T; s *= 2) {
        A.s = s;
        const long long n_elim = lanes * ((T - s + 2 * s - 1) / (2 * s)), n_surv = lanes * ((T + 2 * s - 1) / (2 * s));
        if (rowwise) {
          if ((rc = go(km->fz_m, (n_elim + bpw - 1) / bpw)) || (rc = go(km->fs_m, (n_surv + 63) / 64))) return rc;
        } else if ((rc = go(km->fwd_m, n_surv + n_elim))) return rc;
      }
      if (!rowwise && ne > 0) { A.final_block = 1; if ((rc = go(km->fwd_m, lanes))) return rc; }
      continue;
    }
    A.final_block = 1;
    if ((rc = rowwise ? go(km->fz_m, (lanes + bpw - 1) / bpw) : go(km->bwd_m, lanes))) return rc;
    A.final_block = 0;
    long long top = 1;
    while (top * 2 < T) top *= 2;
    for (long long s = top; s >= 1; s /= 2) {
      if (s >= T) continue;
      A.s = s;
      const long long n_elim = lanes * ((T - s + 2 * s - 1) / (2 * s));
      if ((rc = rowwise ? go(km->bw_m, (n_elim + bpw - 1) / bpw) : go(km->bwd_m, n_elim))) return rc;
    }
  }
  return IEM_OK;
}

/* ---- the dense border on the device (csrc/iem_kkt_border_device.h) ------------------------------------------------------------ */
namespace {
// the code object (the synchronous part of the first call)
int kkt_border_setup(iem_model *m) { return fixed_object(m, F_KBORDER); }
bool kkt_border_shape_ok(int64_t S, int ne, int n_border) { return S >= 1 && ne >= 4 && ne <= 128 && ne % 4 == 0 && n_border >= 0 && n_border <= ne; }
// LDS of kkt_border_ldl / kkt_border_solve (the layout at the head of csrc/iem_kkt_border_device.h)
unsigned kkt_border_lds(int ne) { return (unsigned)(8 * (ne * (ne + 1) + 2 * ne + 16) + 4 * (2 * ne + 16)); }
unsigned kkt_border_wg(int ne) { return ne <= 32 ? 64u : 256u; }
// the column sums' pair of launches for nr matrices of rows x w (matrix u at in + u in_ld) through `fn` (kkt_colsum_m of a chain module
// or its twin kkt_border_colsum): partial rows at part + u part_ld, the sums at part + u part_ld + res_off
int kkt_border_sums(iem_model *m, hipFunction_t fn, const double *in, long long in_ld, int64_t rows, int64_t w, int nr, double *part, long long part_ld, long long res_off) {
  struct Sum { const double *in; double *out; long long rows, w, rows_per_wg, in_ld, out_ld, wgs; };
  const int64_t ncc = (w + 255) / 256, per = (rows + 511) / 512, nrc = (rows + per - 1) / per;
  Sum A{in, part, (long long)rows, (long long)w, (long long)per, in_ld, part_ld, (long long)(nrc * ncc)};
  int rc = kkt_launch_raw(m, fn, &A, sizeof A, nr * nrc * ncc, 256);
  if (rc) return rc;
  Sum B{part, part + res_off, (long long)nrc, (long long)w, (long long)nrc, part_ld, part_ld, (long long)ncc};
  return kkt_launch_raw(m, fn, &B, sizeof B, nr * ncc, 256);
}
// Gs = G - sum_k Gp[k] factorised by ONE workgroup; `part`: 513 ne^2 doubles (res_off = 512 ne^2) or what the caller states
int kkt_border_factor_run(iem_model *m, hipFunction_t colsum, int64_t S, int ne, int n_border, const double *d_G, const double *d_Gp, double *d_F, int32_t *d_piv,
                          int64_t *d_info, double rel, double *part, long long res_off) {
  const int64_t w = (int64_t)ne * ne;
  int rc = kkt_border_sums(m, colsum, d_Gp, w * S, S, w, 1, part, 0, res_off);
  if (rc) return rc;
  struct { const double *G, *gsum; double *F; int *piv; long long *info; int ne, n_border; double rel; } A{d_G, part + res_off, d_F, d_piv, (long long *)d_info, ne, n_border, rel};
  return launch_args(m->fixed[F_KBORDER].fn[KBORDER_LDL], &A, sizeof A, 1, 1, kkt_border_wg(ne), kkt_border_lds(ne), m->stream);
}
struct KktBorderSolveArgsH { const double *F; const int *piv; const double *rhs; const long long *src, *dst; const double *sum; double *xB; long long ld_rhs, ld_sum, ld_x; int ne, n_border; };
int kkt_border_solve_run(iem_model *m, const KktBorderSolveArgsH &a, int nrhs) {
  KktBorderSolveArgsH A = a;
  return launch_args(m->fixed[F_KBORDER].fn[KBORDER_SOLVE], &A, sizeof A, (unsigned)nrhs, 1, kkt_border_wg(a.ne), kkt_border_lds(a.ne), m->stream);
}
int kkt_border_workspace(iem_model *m, int64_t doubles) {
  if (m->kb_part_n >= doubles) return IEM_OK;
  if (m->kb_part) { HIP_TRY(hipStreamSynchronize(m->stream)); hipFree(m->kb_part); m->kb_part = nullptr; m->kb_part_n = 0; }
  HIP_TRY(hipMalloc((void **)&m->kb_part, (size_t)doubles * 8));
  m->kb_part_n = doubles;
  return IEM_OK;
}
}  // namespace

int iem_kkt_border_source(char **out_src, uint64_t *out_key) { return fixed_source_out(F_KBORDER, out_src, out_key); }

int iem_kkt_border_factor(iem_model *m, int64_t S, int ne, int n_border, const double *d_G, const double *d_Gp, double *d_F, int32_t *d_piv, int64_t *d_info,
                          double rel) {
  if (!m || !d_G || !d_Gp || !d_F || !d_piv || !d_info) return fail(IEM_E_ARG, "iem_kkt_border_factor: null argument");
  if (!kkt_border_shape_ok(S, ne, n_border) || !(rel >= 0.0))
    return fail(IEM_E_ARG, "iem_kkt_border_factor: S >= 1, ne a multiple of 4 in 4..128, 0 <= n_border <= ne, rel >= 0");
  DevGuard dg_(m->device);
  int rc = kkt_border_setup(m);
  if (rc) return rc;
  const int64_t w = (int64_t)ne * ne, nrc = std::min<int64_t>(S, 512);      // (at most 512 partial rows, then the result)
  if ((rc = kkt_border_workspace(m, (nrc + 1) * w))) return rc;
  return kkt_border_factor_run(m, m->fixed[F_KBORDER].fn[KBORDER_COLSUM], S, ne, n_border, d_G, d_Gp, d_F, d_piv, d_info, rel, m->kb_part, nrc * w);
}

int iem_kkt_border_solve(iem_model *m, int64_t S, int ne, int n_border, int nrhs, const double *d_F, const int32_t *d_piv, const double *d_rBp, const double *d_rB,
                         double *d_xB) {
  if (!m || !d_F || !d_piv || !d_rBp || !d_rB || !d_xB) return fail(IEM_E_ARG, "iem_kkt_border_solve: null argument");
  if (!kkt_border_shape_ok(S, ne, n_border) || nrhs < 1)
    return fail(IEM_E_ARG, "iem_kkt_border_solve: S >= 1, ne a multiple of 4 in 4..128, 0 <= n_border <= ne, nrhs >= 1");
  DevGuard dg_(m->device);
  int rc = kkt_border_setup(m);
  if (rc) return rc;
  const int64_t nrc = std::min<int64_t>(S, 512), wp = (nrc + 1) * ne;
  if ((rc = kkt_border_workspace(m, (int64_t)nrhs * wp))) return rc;
  if ((rc = kkt_border_sums(m, m->fixed[F_KBORDER].fn[KBORDER_COLSUM], d_rBp, (long long)(S * ne), S, ne, nrhs, m->kb_part, (long long)wp, (long long)(nrc * ne)))) return rc;
  return kkt_border_solve_run(m, KktBorderSolveArgsH{d_F, d_piv, d_rB, nullptr, nullptr, m->kb_part + nrc * ne, d_xB, (long long)ne, (long long)wp, (long long)ne, ne, n_border}, nrhs);
}

/* ---- the chain KKT solver as ONE object behind the C-ABI (what a host without the Python layer binds) ---------------------- */
struct iem_kkt {
  iem_model *m = nullptr;
  iem::KktLayout L;
  iem_model::KktMod *km = nullptr;
  double *d_flat = nullptr, *d_BR = nullptr, *d_Z = nullptr, *d_Gp = nullptr, *d_part = nullptr;
  int32_t *d_rows = nullptr, *d_cols = nullptr;
  long long *d_dest = nullptr, *d_on = nullptr, *d_pos = nullptr, *d_border = nullptr, *d_bloc = nullptr, *d_info = nullptr;
  unsigned *d_seg = nullptr, *d_perm = nullptr;
  int64_t n_dest = 0, n_on = 0, n_h = 0, n_j = 0;
  // The solves' workspace: the block-ordered planes r, z, rBp, xB of ONE chunk of `chunk_cols` columns — one column from
  // iem_kkt_create on, the shape's chunk width from the first multi-column solve on (kkt_chunk_workspace).  Hub mode uses column 0.
  // An allocation per plane, grown together: as planes of one allocation r and z cost the one-column refined solve 1 % at 1e5
  // quadrotor supports (the kernels' own time is the same in a trace; profiles/kkt_single_path_ab.json).
  // (The column sums' partials sit in d_part: 513 ne doubles per column, and a chunk has at most four columns, ne at least four.)
  double *w_r = nullptr, *w_z = nullptr, *w_rBp = nullptr, *w_xB = nullptr;
  int chunk_cols = 0;
  std::vector<double> Gs;        // the border's Schur complement (host), set by iem_kkt_factor
  // The residuals' and the refinement's workspace: the planes p | r | dsol of `ref_cols` columns of nvar + ncon doubles — one column
  // from the first residual or refined call on, one slab from the first such call with several columns on (kkt_refine_workspace)
  double *w_ref = nullptr;
  int ref_cols = 0;
  int border_mode = 0;           // iem_kkt_set_border: 0 the border on the host, 1 on the device (d_F, d_piv: its factors)
  double *d_F = nullptr;
  int32_t *d_piv = nullptr;
  bool factored = false;
  struct KktHub *hub = nullptr;  // hub mode (L.hubs): the span-sparse border's buffers and the library handle of its GEMMs
};

// rocBLAS for the plain library GEMMs / GEMVs of the hubs' Schur complement — loaded on first use (dlopen), so that the library
// does not depend on it for anything else
struct RocBlas {
  void *lib = nullptr, *handle = nullptr;
  int (*create)(void **) = nullptr;
  int (*destroy)(void *) = nullptr;
  int (*set_stream)(void *, hipStream_t) = nullptr;
  int (*dgemm)(void *, int, int, int, int, int, const double *, const double *, int, const double *, int, const double *, double *, int) = nullptr;
  int (*dgemm_sb)(void *, int, int, int, int, int, const double *, const double *, int, long long, const double *, int, long long, const double *, double *, int, long long, int) = nullptr;
  int (*dgemv)(void *, int, int, int, const double *, const double *, int, const double *, int, const double *, double *, int) = nullptr;
  int (*dgemv_sb)(void *, int, int, int, const double *, const double *, int, long long, const double *, int, long long, const double *, double *, int, long long, int) = nullptr;
  int (*dgeam)(void *, int, int, int, int, const double *, const double *, int, const double *, const double *, int, double *, int) = nullptr;
};
struct KktHub {
  RocBlas bl;
  int32_t *d_q = nullptr, *d_qr = nullptr, *d_qc = nullptr;
  double *E[2] = {nullptr, nullptr}, *Z = nullptr, *Sd = nullptr, *Lmat = nullptr, *LT = nullptr, *Dinv = nullptr, *Linv = nullptr, *Nmat = nullptr, *X[2] = {nullptr, nullptr}, *eye96 = nullptr,
         *eyeP = nullptr, *x = nullptr, *w = nullptr, *tmp = nullptr, *r2 = nullptr;
  long long *d_dinfo = nullptr;
  int64_t e_cap = 0, steps = 0, npanels = 0;
};

namespace {
int kkt_upload_bytes(void **d, const void *h, size_t bytes) {
  HIP_TRY(hipMalloc(d, std::max<size_t>(bytes, 8)));
  if (bytes) HIP_TRY(hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice));
  return IEM_OK;
}
#define kkt_upload(dptr, vec) kkt_upload_bytes((void **)(dptr), (vec).data(), (vec).size() * sizeof((vec)[0]))
// column sums of a device S x w matrix, to the host: kkt_border_sums' two launches (up to 512 row chunks x column chunks of 256 —
// every CU busy: the border terms of 1e4 OPF scenarios are 216 MB), then w doubles come home
int kkt_colsum_host(iem_kkt *k, const double *d_in, int64_t rows, int64_t w, std::vector<double> &out) {
  iem_model *m = k->m;
  int rc = kkt_border_sums(m, k->km->colsum_m, d_in, 0, rows, w, 1, k->d_part, 0, (long long)(512 * w));
  if (rc) return rc;
  out.assign((size_t)w, 0.0);
  HIP_TRY(hipStreamSynchronize(m->stream));
  HIP_TRY(hipMemcpy(out.data(), k->d_part + 512 * w, (size_t)w * 8, hipMemcpyDeviceToHost));
  return IEM_OK;
}
// the solves' workspace for `cols` columns (grown, never shrunk: a growth waits for the stream, frees and allocates)
int kkt_chunk_workspace(iem_kkt *k, int cols) {
  if (k->chunk_cols >= cols) return IEM_OK;
  if (k->chunk_cols) HIP_TRY(hipStreamSynchronize(k->m->stream));
  const iem::KktLayout &L = k->L;
  const int64_t ne = std::max<int64_t>(L.ne, 0), doubles[4] = {L.S * L.nb, L.S * L.nb, L.S * ne, ne};
  double **plane[4] = {&k->w_r, &k->w_z, &k->w_rBp, &k->w_xB};
  for (double **p : plane) { if (*p) hipFree(*p); *p = nullptr; }
  k->chunk_cols = 0;
  for (int i = 0; i < 4; ++i) HIP_TRY(hipMalloc((void **)plane[i], (size_t)std::max<int64_t>(cols * doubles[i], 1) * 8));
  k->chunk_cols = cols;
  return IEM_OK;
}
}  // namespace


/* ---- hub mode of the KKT object: a laned 2-D grid whose border is kept as span-sparse hub columns (kkt_chain.HubChainKKT is the
 * Python-held form of the same pipeline; tests compare the two) ---------------------------------------------------------------- */
namespace {
constexpr int HUB_LEAF = 96, HUB_PW = 5 * HUB_LEAF, HUB_CH = 10 * HUB_LEAF, HUB_CLIP = 16;
constexpr int RB_N = 111, RB_T = 112;      // rocblas_operation_none / _transpose
int hub_blas_load(iem_kkt *k) {
  RocBlas &b = k->hub->bl;
  if (b.handle) return b.set_stream(b.handle, k->m->stream) == 0 ? IEM_OK : fail(IEM_E_HIP, "rocblas_set_stream");      // (the handle's stream may have been changed since)
  b.lib = dlopen("librocblas.so", RTLD_NOW | RTLD_GLOBAL);
  if (!b.lib) b.lib = dlopen("/opt/rocm/lib/librocblas.so", RTLD_NOW | RTLD_GLOBAL);
  if (!b.lib) return fail(IEM_E_HIP, std::string("chain KKT (hub border): cannot load librocblas.so (") + dlerror() + ")");
  auto sym = [&](const char *n) { return dlsym(b.lib, n); };
  b.create = (decltype(b.create))sym("rocblas_create_handle");
  b.destroy = (decltype(b.destroy))sym("rocblas_destroy_handle");
  b.set_stream = (decltype(b.set_stream))sym("rocblas_set_stream");
  b.dgemm = (decltype(b.dgemm))sym("rocblas_dgemm");
  b.dgemm_sb = (decltype(b.dgemm_sb))sym("rocblas_dgemm_strided_batched");
  b.dgemv = (decltype(b.dgemv))sym("rocblas_dgemv");
  b.dgemv_sb = (decltype(b.dgemv_sb))sym("rocblas_dgemv_strided_batched");
  b.dgeam = (decltype(b.dgeam))sym("rocblas_dgeam");
  if (!b.create || !b.destroy || !b.set_stream || !b.dgemm || !b.dgemm_sb || !b.dgemv || !b.dgemv_sb || !b.dgeam) return fail(IEM_E_HIP, "chain KKT (hub border): librocblas.so lacks an entry point");
  if (b.create(&b.handle) != 0) return fail(IEM_E_HIP, "rocblas_create_handle");
  if (b.set_stream(b.handle, k->m->stream) != 0) return fail(IEM_E_HIP, "rocblas_set_stream");
  return IEM_OK;
}
#define RB_TRY(call) do { if ((call) != 0) return fail(IEM_E_HIP, "rocBLAS call failed: " #call); } while (0)
// ROW-MAJOR  C[m x n] = alpha op(A) op(B) + beta C   through the column-major library (C' = op(B)' op(A)')
int gemm_rm(iem_kkt *k, bool ta, bool tb, int64_t m, int64_t n, int64_t kk, double alpha, const double *A, int64_t lda, const double *B, int64_t ldb, double beta, double *C, int64_t ldc) {
  if (m <= 0 || n <= 0) return IEM_OK;
  RB_TRY(k->hub->bl.dgemm(k->hub->bl.handle, tb ? RB_T : RB_N, ta ? RB_T : RB_N, (int)n, (int)m, (int)kk, &alpha, B, (int)ldb, A, (int)lda, &beta, C, (int)ldc));
  return IEM_OK;
}
// ROW-MAJOR  y = alpha op(A) x + beta y,  A [m x n]
int gemv_rm(iem_kkt *k, bool ta, int64_t m, int64_t n, double alpha, const double *A, int64_t lda, const double *x, double beta, double *y) {
  if (m <= 0 || n <= 0) return IEM_OK;
  RB_TRY(k->hub->bl.dgemv(k->hub->bl.handle, ta ? RB_N : RB_T, (int)n, (int)m, &alpha, A, (int)lda, x, 1, &beta, y, 1));
  return IEM_OK;
}
int copy2d(iem_kkt *k, double *dst, int64_t ldd, const double *src, int64_t lds, int64_t rows, int64_t cols) {
  if (rows <= 0 || cols <= 0) return IEM_OK;
  HIP_TRY(hipMemcpy2DAsync(dst, (size_t)ldd * 8, src, (size_t)lds * 8, (size_t)cols * 8, (size_t)rows, hipMemcpyDeviceToDevice, k->m->stream));
  return IEM_OK;
}
// Sv -= A' Z  (symmetric; Sv: w x w at hub h0 of the Schur complement, row length ld; A, Z: K x w, row length ldw): wide products only
// into the block lower triangle, column chunks cut at the multiples of HUB_CH hubs (the pivot blocks of the LDL' never straddle them)
int hub_sub_lower(iem_kkt *k, double *Sv, int64_t ld, const double *A, const double *Z, int64_t ldw, int64_t K, int64_t w, int64_t h0) {
  if (w <= 2 * HUB_CH) return gemm_rm(k, true, false, w, w, K, -1.0, A, ldw, Z, ldw, 1.0, Sv, ld);
  int64_t c0 = 0;
  while (c0 < w) {
    const int64_t c1 = std::min<int64_t>(w, ((h0 + c0) / HUB_CH + 1) * HUB_CH - h0);
    int rc = gemm_rm(k, true, false, w - c0, c1 - c0, K, -1.0, A + c0, ldw, Z + c0, ldw, 1.0, Sv + c0 * ld + c0, ld);
    if (rc) return rc;
    c0 = c1;
  }
  return IEM_OK;
}
int hub_level_launch(iem_kkt *k, int64_t s, const double *E, double *Z, double *En, int last) {
  const iem::KktLayout &L = k->L;
  return iem_kkt_hub_level(k->m, L.S, L.Tp, L.nb, L.nc, k->d_flat + L.oD(), k->d_flat + L.oB(), k->hub->d_q, L.nq, k->hub->d_qr, L.nr, k->hub->d_qc, L.ncq, (int)L.hw, s, E, Z, En, last);
}
int hub_alloc(iem_kkt *k) {
  const iem::KktLayout &L = k->L;
  KktHub *h = k->hub = new KktHub;
  int rc;
  if ((rc = kkt_upload(&h->d_q, L.Q)) || (rc = kkt_upload(&h->d_qr, L.qR)) || (rc = kkt_upload(&h->d_qc, L.qC))) return rc;
  const int64_t per = L.lanes * L.nq;
  int64_t cap = L.Tp * L.hw, P = 1;
  for (int64_t s = 1; s < L.Tp; s *= 2) {
    const int64_t alive = (L.Tp + s - 1) / s, ns = alive - alive / 2;
    cap = std::max(cap, std::max(alive * (2 * s - 1), ns * (4 * s - 1)) * L.hw);
    P = 2 * s;
  }
  cap = std::max(cap, (2 * P - 1) * L.hw);
  h->e_cap = cap * per;
  for (int i = 0; i < 2; ++i) HIP_TRY(hipMalloc((void **)&h->E[i], (size_t)h->e_cap * 8));
  HIP_TRY(hipMalloc((void **)&h->Z, (size_t)h->e_cap * 8));
  const int64_t H = L.H;
  h->steps = (H + HUB_LEAF - 1) / HUB_LEAF; h->npanels = (H + HUB_PW - 1) / HUB_PW;
  HIP_TRY(hipMalloc((void **)&h->Sd, (size_t)(H * H) * 8));
  HIP_TRY(hipMalloc((void **)&h->Lmat, (size_t)(H * H) * 8));      // L (the scaled columns); Sd keeps L D, the columns before scaling
  HIP_TRY(hipMalloc((void **)&h->LT, (size_t)(H * H) * 8));        // L' panel by panel: the backward substitution reads rows, like the forward one
  HIP_TRY(hipMalloc((void **)&h->Dinv, (size_t)(h->steps * HUB_LEAF * HUB_LEAF) * 8));
  HIP_TRY(hipMalloc((void **)&h->Linv, (size_t)(h->npanels * HUB_PW * HUB_PW) * 8));
  HIP_TRY(hipMalloc((void **)&h->Nmat, (size_t)(HUB_PW * HUB_PW) * 8));
  for (int i = 0; i < 2; ++i) HIP_TRY(hipMalloc((void **)&h->X[i], (size_t)(HUB_PW * HUB_PW) * 8));
  std::vector<double> eye((size_t)(HUB_PW * HUB_PW), 0.0), eye96((size_t)(HUB_LEAF * HUB_LEAF), 0.0);
  for (int i = 0; i < HUB_PW; ++i) eye[(size_t)(i * HUB_PW + i)] = 1.0;
  for (int i = 0; i < HUB_LEAF; ++i) eye96[(size_t)(i * HUB_LEAF + i)] = 1.0;
  if ((rc = kkt_upload(&h->eyeP, eye)) || (rc = kkt_upload(&h->eye96, eye96))) return rc;
  const int64_t hv = std::max<int64_t>(h->steps * HUB_LEAF, L.Tp * L.hw);
  HIP_TRY(hipMalloc((void **)&h->x, (size_t)hv * 8));
  HIP_TRY(hipMalloc((void **)&h->w, (size_t)hv * 8));
  HIP_TRY(hipMalloc((void **)&h->tmp, (size_t)HUB_PW * 8));
  HIP_TRY(hipMalloc((void **)&h->r2, (size_t)(L.S * L.nb) * 8));
  HIP_TRY(hipMalloc((void **)&h->d_dinfo, (size_t)(h->steps * 3) * 8));
  return IEM_OK;
}
void hub_free(iem_kkt *k) {
  KktHub *h = k->hub;
  if (!h) return;
  for (void *p : {(void *)h->d_q, (void *)h->d_qr, (void *)h->d_qc, (void *)h->E[0], (void *)h->E[1], (void *)h->Z, (void *)h->Sd, (void *)h->Lmat, (void *)h->LT, (void *)h->Dinv, (void *)h->Linv,
                  (void *)h->Nmat, (void *)h->X[0], (void *)h->X[1], (void *)h->eye96, (void *)h->eyeP, (void *)h->x, (void *)h->w, (void *)h->tmp, (void *)h->r2, (void *)h->d_dinfo})
    if (p) hipFree(p);
  if (h->bl.handle && h->bl.destroy) h->bl.destroy(h->bl.handle);
  delete h;
  k->hub = nullptr;
}
// the hubs' Schur complement Sd (H x H, row-major, lower triangle + the pivot blocks' squares valid): block LDL' in panels of HUB_PW,
// pivot blocks of HUB_LEAF inverted by kkt_eliminate (which counts their pivot signs).  Sd keeps the columns BEFORE scaling (L D),
// Lmat receives L = (L D) D^-1 — the updates are L (L D)': no copy of a panel is ever needed — and LT its transpose, panel by panel.
int hub_dense_factor(iem_kkt *k) {
  const iem::KktLayout &L = k->L;
  KktHub *h = k->hub;
  iem_model *m = k->m;
  const int64_t n = L.H;
  double *Sd = h->Sd, *Lm = h->Lmat;
  int rc;
  iem_model::KktMod *leaf = nullptr;
  if ((rc = kkt_module(m, HUB_LEAF, -1, 4, &leaf))) return rc;
  HIP_TRY(hipMemsetAsync(h->d_dinfo, 0, (size_t)(h->steps * 3) * 8, m->stream));
  // pivot threshold of the hubs' blocks: RELATIVE to the largest diagonal entry of their Schur complement — a pivot at rounding level of
  // that scale is neither sign and is reported as doubtful (as the dense border's near-zero eigenvalues are: ADVICE r03), not as positive
  double tiny = 1e-30;
  {
    struct { const double *S; double *out; long long n, ld; } A{Sd, h->tmp, (long long)n, (long long)n};
    if ((rc = kkt_launch_raw(m, k->km->hub_diagmax, &A, sizeof A, 1, 256))) return rc;
    double dmax = 0.0;
    HIP_TRY(hipStreamSynchronize(m->stream));
    HIP_TRY(hipMemcpy(&dmax, h->tmp, 8, hipMemcpyDeviceToHost));
    if (dmax > 0.0 && std::isfinite(dmax)) tiny = std::max(tiny, 1e-14 * dmax);
  }
  for (int64_t p0 = 0, pi = 0; p0 < n; p0 += HUB_PW, ++pi) {
    const int64_t p1 = std::min<int64_t>(p0 + HUB_PW, n), pw = p1 - p0;
    for (int64_t kk = p0; kk < p1; kk += HUB_LEAF) {
      const int64_t e = std::min<int64_t>(kk + HUB_LEAF, p1), w = e - kk, ki = kk / HUB_LEAF;
      double *blk = h->Dinv + ki * HUB_LEAF * HUB_LEAF;
      { struct { const double *src; double *dst; long long ld; int w, nb; } A{Sd + kk * n + kk, blk, (long long)n, (int)w, HUB_LEAF};
        if ((rc = kkt_launch_raw(m, k->km->hub_leaf, &A, sizeof A, (HUB_LEAF * HUB_LEAF + 255) / 256, 256))) return rc; }
      {   // in-place inverse + pivot signs: one block, no chain, no border
        KktArgsH A{blk, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, h->d_dinfo + 3 * ki, 1, 1, 2, tiny};
        if ((rc = kkt_launch_elim(m, leaf, A, 1))) return rc;
      }
      if (e < n) {
        if ((rc = gemm_rm(k, false, false, n - e, w, w, 1.0, Sd + e * n + kk, n, blk, HUB_LEAF, 0.0, Lm + e * n + kk, n))) return rc;                       // L = (L D) D^-1
        if (e < p1 && (rc = gemm_rm(k, false, true, n - e, p1 - e, w, -1.0, Lm + e * n + kk, n, Sd + e * n + kk, n, 1.0, Sd + e * n + e, n))) return rc;    // the panel's own columns
      }
    }
    {   // the panel's unit lower triangle L_pp = I + N (N strictly block lower: N^5 = 0), inverted once: (I + N)^-1 = I - N (I - N (I - ...))
      struct { const double *src; double *N, *X; long long ld; int pw, ldp, leaf; } A{Lm + p0 * n + p0, h->Nmat, h->X[0], (long long)n, (int)pw, HUB_PW, HUB_LEAF};
      if ((rc = kkt_launch_raw(m, k->km->hub_mask, &A, sizeof A, (pw * pw + 255) / 256, 256))) return rc;
      int cur = 0;
      for (int64_t it = 0; it < (pw - 1) / HUB_LEAF - 1; ++it) {
        HIP_TRY(hipMemcpyAsync(h->X[1 - cur], h->eyeP, (size_t)(HUB_PW * HUB_PW) * 8, hipMemcpyDeviceToDevice, m->stream));
        if ((rc = gemm_rm(k, false, false, pw, pw, pw, -1.0, h->Nmat, HUB_PW, h->X[cur], HUB_PW, 1.0, h->X[1 - cur], HUB_PW))) return rc;
        cur = 1 - cur;
      }
      HIP_TRY(hipMemcpyAsync(h->Linv + pi * HUB_PW * HUB_PW, h->X[cur], (size_t)(HUB_PW * HUB_PW) * 8, hipMemcpyDeviceToDevice, m->stream));
    }
    if (p1 < n) {   // LT[p0:p1, p1:] = L[p1:, p0:p1]'  (column-major view: C ((n - p1) x pw) = A' with A = the pw x (n - p1) view of the panel)
      const double one = 1.0, zero = 0.0;
      RB_TRY(h->bl.dgeam(h->bl.handle, RB_T, RB_N, (int)(n - p1), (int)pw, &one, Lm + p1 * n + p0, (int)n, &zero, h->LT + p0 * n + p1, (int)n, h->LT + p0 * n + p1, (int)n));
    }
    for (int64_t c0 = p1; c0 < n; c0 += HUB_CH) {   // the rest of the matrix, lower triangle only, once per panel (inner dimension = the panel's width)
      const int64_t c1 = std::min<int64_t>(c0 + HUB_CH, n);
      if ((rc = gemm_rm(k, false, true, n - c0, c1 - c0, pw, -1.0, Lm + c0 * n + p0, n, Sd + c0 * n + p0, n, 1.0, Sd + c0 * n + c0, n))) return rc;
    }
  }
  return IEM_OK;
}
// x (H) in place: S x = b with the factors above
int hub_dense_solve(iem_kkt *k, double *x) {
  const iem::KktLayout &L = k->L;
  KktHub *h = k->hub;
  iem_model *m = k->m;
  const int64_t n = L.H;
  int rc;
  for (int64_t p0 = 0, pi = 0; p0 < n; p0 += HUB_PW, ++pi) {       // L z = b
    const int64_t p1 = std::min<int64_t>(p0 + HUB_PW, n), pw = p1 - p0;
    if ((rc = gemv_rm(k, false, pw, pw, 1.0, h->Linv + pi * HUB_PW * HUB_PW, HUB_PW, x + p0, 0.0, h->tmp))) return rc;
    HIP_TRY(hipMemcpyAsync(x + p0, h->tmp, (size_t)pw * 8, hipMemcpyDeviceToDevice, m->stream));
    if (p1 < n && (rc = gemv_rm(k, false, n - p1, pw, -1.0, h->Lmat + p1 * n + p0, n, x + p0, 1.0, x + p1))) return rc;
  }
  {   // D^-1: one 96 x 96 product per pivot block (x is padded up to the last whole block with zeros)
    const double one = 1.0, zero = 0.0;
    if (h->steps * HUB_LEAF > n) HIP_TRY(hipMemsetAsync(x + n, 0, (size_t)(h->steps * HUB_LEAF - n) * 8, m->stream));
    RB_TRY(h->bl.dgemv_sb(h->bl.handle, RB_T, HUB_LEAF, HUB_LEAF, &one, h->Dinv, HUB_LEAF, (long long)HUB_LEAF * HUB_LEAF, x, 1, HUB_LEAF, &zero, h->w, 1, HUB_LEAF, (int)h->steps));
  }
  double *w = h->w;
  for (int64_t pi = h->npanels - 1; pi >= 0; --pi) {               // L' x = w  (rows of LT: the same fast matrix-vector kernel as on the way down)
    const int64_t p0 = pi * HUB_PW, p1 = std::min<int64_t>(p0 + HUB_PW, n), pw = p1 - p0;
    if (p1 < n && (rc = gemv_rm(k, false, pw, n - p1, -1.0, h->LT + p0 * n + p1, n, w + p1, 1.0, w + p0))) return rc;
    if ((rc = gemv_rm(k, true, pw, pw, 1.0, h->Linv + pi * HUB_PW * HUB_PW, HUB_PW, w + p0, 0.0, h->tmp))) return rc;
    HIP_TRY(hipMemcpyAsync(w + p0, h->tmp, (size_t)pw * 8, hipMemcpyDeviceToDevice, m->stream));
  }
  HIP_TRY(hipMemcpyAsync(x, w, (size_t)n * 8, hipMemcpyDeviceToDevice, m->stream));
  return IEM_OK;
}
int hub_factor(iem_kkt *k, int64_t *out_inertia) {
  const iem::KktLayout &L = k->L;
  KktHub *h = k->hub;
  iem_model *m = k->m;
  int rc;
  if ((rc = hub_blas_load(k))) return rc;
  double *D = k->d_flat + L.oD(), *Bt = k->d_flat + L.oB(), *E0 = k->d_flat + L.oE(), *Sbig = k->d_flat + L.oG();
  const int64_t Tp = L.Tp, hw = L.hw, Hp = L.Hp, H = L.H, K = L.lanes * L.nq;
  auto level = [&](int64_t s, int what) { return iem_kkt_chain_level(m, L.S, Tp, L.nb, L.nc, D, Bt, k->d_BR, k->d_rows, k->d_cols, (int64_t *)k->d_info, 1e-30, s, what); };
  if ((rc = level(1, 3))) return rc;
  HIP_TRY(hipMemcpyAsync(h->E[0], E0, (size_t)(Tp * K * hw) * 8, hipMemcpyDeviceToDevice, m->stream));
  int cur = 0;
  int64_t s = 1;
  for (; s < Tp; s *= 2) {
    if ((rc = level(s, 0))) return rc;                                      // D of the blocks t = (2a+1)s now holds their inverses
    const int64_t alive = (Tp + s - 1) / s, n_e = alive / 2, W = (2 * s - 1) * hw;
    const double *E = h->E[cur];
    if ((rc = hub_level_launch(k, s, E, h->Z, h->E[1 - cur], 0))) return rc;   // Z = D^-1[Q, Q] E of the eliminated, the survivors' widened columns
    if (n_e > HUB_CLIP) {                                                     // many small intervals: one batched product onto disjoint diagonal blocks of S
      const double alpha = -1.0, beta = 1.0;
      // row-major C_i -= A_i' Z_i  ==  column-major  C_i' -= Z_i(c) A_i(c)'   with X(c) = X' (W x K, leading dimension W)
      RB_TRY(h->bl.dgemm_sb(h->bl.handle, RB_N, RB_T, (int)W, (int)W, (int)K, &alpha, h->Z, (int)W, (long long)(K * W), E + K * W, (int)W, (long long)(2 * K * W), &beta,
                            Sbig + hw * (Hp + 1), (int)Hp, (long long)(2 * s * hw * (Hp + 1)), (int)n_e));
    } else {                                                                  // few wide ones: clipped to the hubs that exist
      for (int64_t mi = 0; mi < n_e; ++mi) {
        const int64_t te = (2 * mi + 1) * s, h0 = (te - s + 1) * hw, w = std::min<int64_t>(W, H - h0);
        if (w <= 0) continue;
        if ((rc = hub_sub_lower(k, Sbig + h0 * (Hp + 1), Hp, E + (2 * mi + 1) * K * W, h->Z + mi * K * W, W, K, w, h0))) return rc;
      }
    }
    cur = 1 - cur;
    if ((rc = level(s, 1))) return rc;                                      // fold the inverses into the survivors' blocks and couplings
  }
  // one block per lane is left (t = 0), coupled to every hub (s is the power of two the levels stopped at)
  if ((rc = level(1, 2))) return rc;
  {
    const int64_t W = (2 * s - 1) * hw;
    if ((rc = hub_level_launch(k, s, h->E[cur], h->Z, nullptr, 1))) return rc;
    if ((rc = hub_sub_lower(k, Sbig, Hp, h->E[cur] + (s - 1) * hw, h->Z + (s - 1) * hw, W, K, H, 0))) return rc;
  }
  if ((rc = copy2d(k, h->Sd, H, Sbig, Hp, H, H))) return rc;
  if ((rc = hub_dense_factor(k))) return rc;
  long long info[3] = {0, 0, 0};
  std::vector<long long> dinfo((size_t)(h->steps * 3));
  HIP_TRY(hipStreamSynchronize(m->stream));
  HIP_TRY(hipMemcpy(info, k->d_info, 24, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(dinfo.data(), h->d_dinfo, dinfo.size() * 8, hipMemcpyDeviceToHost));
  int64_t neg = info[0], doubtful = info[1];
  for (int64_t i = 0; i < h->steps; ++i) { neg += dinfo[(size_t)(3 * i)]; doubtful += dinfo[(size_t)(3 * i + 1)]; }
  k->factored = true;
  if (out_inertia) { out_inertia[0] = L.nvar + L.ncon - neg; out_inertia[1] = neg; out_inertia[2] = doubtful; }
  return IEM_OK;
}
int hub_solve(iem_kkt *k, const double *d_rhs, double *d_sol) {
  const iem::KktLayout &L = k->L;
  KktHub *h = k->hub;
  iem_model *m = k->m;
  int rc;
  if ((rc = hub_blas_load(k))) return rc;
  const double *Dinv = k->d_flat + L.oD(), *Bt = k->d_flat + L.oB(), *E0 = k->d_flat + L.oE();
  struct Vec { const double *E0, *v; double *out; const int *q; long long T, lanes; int nb, nq, hw; };
  auto move = [&](double *dst, const double *src, const long long *di, const long long *si, int64_t cnt) {      // kkt_move_m on one column
    struct { double *dst; const double *src; const long long *di, *si; long long n, ldd, lds; int nr; } A{dst, src, di, si, (long long)cnt, 0, 0, 1};
    return kkt_launch_raw(m, k->km->move_m, &A, sizeof A, (cnt + 255) / 256, 256);
  };
  double *d_r = k->w_r, *d_z = k->w_z;      // column 0 of the solves' workspace
  const size_t rbytes = (size_t)(L.S * L.nb) * 8;
  auto chain = [&](double *r) {
    int e = iem_kkt_chain_solve_lanes(m, L.S, L.Tp, L.nb, 0, L.nc, Dinv, Bt, k->d_BR, k->d_rows, k->d_cols, nullptr, r, d_z, nullptr, nullptr, 0);
    return e ? e : iem_kkt_chain_solve_lanes(m, L.S, L.Tp, L.nb, 0, L.nc, Dinv, Bt, k->d_BR, k->d_rows, k->d_cols, nullptr, r, d_z, nullptr, nullptr, 1);
  };
  HIP_TRY(hipMemsetAsync(h->r2, 0, rbytes, m->stream));
  if ((rc = move(h->r2, d_rhs, k->d_pos, k->d_on, k->n_on))) return rc;
  HIP_TRY(hipMemcpyAsync(d_r, h->r2, rbytes, hipMemcpyDeviceToDevice, m->stream));
  if ((rc = chain(d_r))) return rc;                                          // y = K_c^-1 r_c
  // r_B - E' y on the hubs, the dense solve, then x_c = K_c^-1 (r_c - E x_B)
  HIP_TRY(hipMemsetAsync(h->x, 0, (size_t)std::max<int64_t>(h->steps * HUB_LEAF, L.Tp * L.hw) * 8, m->stream));
  if ((rc = move(h->x, d_rhs, k->d_bloc, k->d_border, L.n_border))) return rc;
  { Vec A{E0, d_r, h->x, h->d_q, (long long)L.Tp, (long long)L.lanes, L.nb, L.nq, (int)L.hw}; if ((rc = kkt_launch_raw(m, k->km->hub_ety, &A, sizeof A, L.Tp, 64))) return rc; }
  if ((rc = hub_dense_solve(k, h->x))) return rc;
  if (L.Tp * L.hw > L.H) HIP_TRY(hipMemsetAsync(h->x + L.H, 0, (size_t)(L.Tp * L.hw - L.H) * 8, m->stream));
  { Vec A{E0, h->x, h->r2, h->d_q, (long long)L.Tp, (long long)L.lanes, L.nb, L.nq, (int)L.hw};
    if ((rc = kkt_launch_raw(m, k->km->hub_ex, &A, sizeof A, (L.Tp * L.lanes * L.nq + 255) / 256, 256))) return rc; }
  if ((rc = chain(h->r2))) return rc;
  if ((rc = move(d_sol, h->r2, k->d_on, k->d_pos, k->n_on))) return rc;
  return move(d_sol, h->x, k->d_border, k->d_bloc, L.n_border);
}
}  // namespace

static void kkt_fill_info(const iem::KktLayout &L, iem_kkt_info_t *out) {
  out->S = L.S; out->n = L.nvar + L.ncon; out->n_border = L.n_border; out->nb = L.nb; out->ne = L.ne; out->nc = L.nc;
  out->reach = L.reach; out->group = L.group; out->phase = L.phase; out->block_doubles = L.total();
  out->lanes = L.lanes; out->hub_ld = L.Hp; out->hubs = L.hubs ? 1 : 0; out->hub_rows = L.nq; out->hubs_per_block = (int32_t)L.hw; out->reserved_ = 0;
}

int iem_kkt_analyse_blob(const void *blob, size_t nbytes, int group, iem_kkt_info_t *info, int64_t **out_blk, int64_t **out_loc, int32_t **out_rows,
                         int32_t **out_cols, int64_t **out_dest, uint32_t **out_seg, uint32_t **out_perm, int64_t *out_n_dest, int64_t *out_n_perm) {
  if (!blob || !info) return fail(IEM_E_ARG, "null argument");
  try {
    iem::Model M;
    iem::parse_blob(blob, nbytes, M);
    std::vector<int64_t> jr((size_t)M.nnzj), jc((size_t)M.nnzj), hr((size_t)M.nnzh), hc((size_t)M.nnzh);
    jac_structure_host(M, jr.data(), jc.data(), 0);
    hess_structure_host(M, hr.data(), hc.data(), 0);
    iem::KktLayout L = iem::kkt_layout(M, jr, jc, hr, hc, group, 96, 128, 48, true);
    iem::KktPlan P = iem::kkt_plan(L, hr, hc, jr, jc);
    kkt_fill_info(L, info);
    auto dup = [](const void *src, size_t bytes) { void *p = std::malloc(std::max<size_t>(bytes, 8)); if (bytes) std::memcpy(p, src, bytes); return p; };
    if (out_blk) *out_blk = (int64_t *)dup(L.blk.data(), L.blk.size() * 8);
    if (out_loc) *out_loc = (int64_t *)dup(L.loc.data(), L.loc.size() * 8);
    if (out_rows) *out_rows = (int32_t *)dup(L.rowsR.data(), L.rowsR.size() * 4);
    if (out_cols) *out_cols = (int32_t *)dup(L.colsC.data(), L.colsC.size() * 4);
    if (out_dest) *out_dest = (int64_t *)dup(P.dest.data(), P.dest.size() * 8);
    if (out_seg) *out_seg = (uint32_t *)dup(P.seg.data(), P.seg.size() * 4);
    if (out_perm) *out_perm = (uint32_t *)dup(P.perm.data(), P.perm.size() * 4);
    if (out_n_dest) *out_n_dest = (int64_t)P.dest.size();
    if (out_n_perm) *out_n_perm = (int64_t)P.perm.size();
  } catch (const std::exception &e) {
    return fail(IEM_E_ARG, e.what());
  }
  return IEM_OK;
}

int iem_kkt_create(iem_model *m, int group, iem_kkt **out) {
  if (!m || !out) return fail(IEM_E_ARG, "null argument");
  if (m->sharded) return fail(IEM_E_ARG, "iem_kkt_create: a sharded handle holds one rank's window; the chain solver wants the whole model");
  DevGuard dg_(m->device);
  struct Drop { void operator()(iem_kkt *p) const { iem_kkt_destroy(p); } };     // (a failed create frees what it had uploaded)
  std::unique_ptr<iem_kkt, Drop> k(new iem_kkt);
  k->m = m;
  try {
    const iem::Model &M = m->model;
    std::vector<int64_t> jr((size_t)M.nnzj), jc((size_t)M.nnzj), hr((size_t)M.nnzh), hc((size_t)M.nnzh);
    jac_structure_host(M, jr.data(), jc.data(), 0);
    if (m->opt.hess_merge) return fail(IEM_E_ARG, "iem_kkt_create: the merged Hessian layout is not supported here");
    hess_structure_host(M, hr.data(), hc.data(), 0);
    k->L = iem::kkt_layout(M, jr, jc, hr, hc, group, 96, 128, 48, true);
    if (!kkt_fits(k->L.nb, k->L.ne, k->L.nc)) return fail(IEM_E_ARG, "chain KKT: the tiles of a block do not fit the LDS of a CU");
    iem::KktPlan P = iem::kkt_plan(k->L, hr, hc, jr, jc);
    k->n_dest = (int64_t)P.dest.size(); k->n_h = P.n_h; k->n_j = P.n_j;
    int rc = kkt_module(m, k->L.nb, k->L.ne, k->L.nc, &k->km);
    if (rc) return rc;
    const iem::KktLayout &L = k->L;
    if (L.ne > 0 && k->km->many_r > L.ne) return fail(IEM_E_ARG, "iem_kkt_create: internal — a chunk of columns is wider than the border");      // (d_part holds a chunk's column sums)
    std::vector<long long> dest(P.dest.begin(), P.dest.end()), on, pos, border, bloc;
    for (int64_t u = 0; u < L.nvar + L.ncon; ++u) {
      if (L.blk[(size_t)u] >= 0) { on.push_back(u); pos.push_back(L.blk[(size_t)u] * L.nb + L.loc[(size_t)u]); }
      else { border.push_back(u); bloc.push_back(L.hubs ? L.hub_of[(size_t)u] : L.loc[(size_t)u]); }
    }
    k->n_on = (int64_t)on.size();
    if ((rc = kkt_upload(&k->d_dest, dest)) || (rc = kkt_upload(&k->d_seg, P.seg)) || (rc = kkt_upload(&k->d_perm, P.perm)) || (rc = kkt_upload(&k->d_on, on)) ||
        (rc = kkt_upload(&k->d_pos, pos)) || (rc = kkt_upload(&k->d_border, border)) || (rc = kkt_upload(&k->d_bloc, bloc)) ||
        (rc = kkt_upload(&k->d_rows, L.rowsR)) || (rc = kkt_upload(&k->d_cols, L.colsC)))
      return rc;
    const int64_t S = L.S, nb = L.nb, ne = L.ne, nc = L.nc;
    HIP_TRY(hipMalloc((void **)&k->d_flat, (size_t)L.total() * 8));
    HIP_TRY(hipMalloc((void **)&k->d_BR, (size_t)std::max<int64_t>(S * nc * nc, 1) * 8));
    HIP_TRY(hipMalloc((void **)&k->d_Z, (size_t)std::max<int64_t>(S * nb * ne, 1) * 8));
    HIP_TRY(hipMalloc((void **)&k->d_Gp, (size_t)std::max<int64_t>(S * ne * ne, 1) * 8));
    if ((rc = kkt_chunk_workspace(k.get(), 1))) return rc;      // (here, not in the first solve: a one-column solve can be captured without a warm-up call)
    HIP_TRY(hipMalloc((void **)&k->d_part, (size_t)(513 * std::max<int64_t>(ne * ne, 1)) * 8));      // kkt_border_sums: 512 partial rows + the result of Gp's sum (ne^2 wide) — and, in a solve, of rBp's per column of a chunk (ne wide, at most ne columns)
    HIP_TRY(hipMalloc((void **)&k->d_info, 32));
    HIP_TRY(hipMalloc((void **)&k->d_F, (size_t)std::max<int64_t>(ne * ne, 1) * 8));
    HIP_TRY(hipMalloc((void **)&k->d_piv, (size_t)std::max<int64_t>(ne, 1) * 4));
    if (L.hubs && (rc = hub_alloc(k.get()))) return rc;
    // the gather / residual / add of the object itself: loaded here, so that iem_kkt_assemble stays launch-only — and behind the
    // allocations, where the lazy load of the former per-row calls sat
    if ((rc = fixed_object(m, F_KDIAG))) return rc;
  } catch (const std::exception &e) {
    return fail(IEM_E_ARG, e.what());
  }
  *out = k.release();
  return IEM_OK;
}

int iem_kkt_destroy(iem_kkt *k) {
  if (!k) return IEM_OK;
  DevGuard dg_(k->m->device);
  hub_free(k);
  for (void *p : {(void *)k->d_flat, (void *)k->d_BR, (void *)k->d_Z, (void *)k->d_Gp, (void *)k->d_part, (void *)k->w_r, (void *)k->w_z, (void *)k->w_rBp, (void *)k->w_xB, (void *)k->w_ref, (void *)k->d_F, (void *)k->d_piv,
                  (void *)k->d_rows, (void *)k->d_cols, (void *)k->d_dest, (void *)k->d_on, (void *)k->d_pos, (void *)k->d_border, (void *)k->d_bloc, (void *)k->d_info,
                  (void *)k->d_seg, (void *)k->d_perm})
    if (p) hipFree(p);
  delete k;
  return IEM_OK;
}

int iem_kkt_info(const iem_kkt *k, iem_kkt_info_t *out) {
  if (!k || !out) return fail(IEM_E_ARG, "null argument");
  const iem::KktLayout &L = k->L;
  kkt_fill_info(L, out);
  return IEM_OK;
}

int iem_kkt_layout(const iem_kkt *k, int64_t *h_blk, int64_t *h_loc, int32_t *h_rows, int32_t *h_cols) {
  if (!k) return fail(IEM_E_ARG, "null argument");
  const iem::KktLayout &L = k->L;
  if (h_blk) std::copy(L.blk.begin(), L.blk.end(), h_blk);
  if (h_loc) std::copy(L.loc.begin(), L.loc.end(), h_loc);
  if (h_rows) std::copy(L.rowsR.begin(), L.rowsR.end(), h_rows);
  if (h_cols) std::copy(L.colsC.begin(), L.colsC.end(), h_cols);
  return IEM_OK;
}

int iem_kkt_assemble(iem_kkt *k, const double *d_hess, const double *d_jac, const double *d_sigma, double delta_w, double delta_c) {
  return iem_kkt_assemble_diag(k, d_hess, d_jac, d_sigma, nullptr, delta_w, delta_c);
}

namespace {
// the launches of a factorisation: the chain's levels and — device border — the column sum of Gp and kkt_border_ldl behind them
int kkt_factor_launch(iem_kkt *k) {
  iem_model *m = k->m;
  const iem::KktLayout &L = k->L;
  const bool chained = L.reach > 0;
  double *D = k->d_flat + L.oD(), *Bt = k->d_flat + L.oB(), *E = k->d_flat + L.oE();
  int rc = iem_kkt_chain_factor(m, L.S, L.nb, L.ne, L.nc, D, chained ? Bt : nullptr, chained ? k->d_BR : nullptr, chained ? k->d_rows : nullptr,
                                chained ? k->d_cols : nullptr, E, k->d_Z, k->d_Gp, (int64_t *)k->d_info, 1e-30);
  if (rc || L.ne <= 0 || k->border_mode != 1) return rc;
  return kkt_border_factor_run(m, k->km->colsum_m, L.S, L.ne, (int)L.n_border, k->d_flat + L.oG(), k->d_Gp, k->d_F, k->d_piv, (int64_t *)k->d_info, 1e-14, k->d_part,
                               512LL * L.ne * L.ne);
}
}  // namespace

int iem_kkt_set_border(iem_kkt *k, int mode) {
  if (!k || (mode != 0 && mode != 1)) return fail(IEM_E_ARG, "iem_kkt_set_border: mode 0 (host) or 1 (device)");
  if (k->L.hubs || k->L.ne <= 0 || mode == k->border_mode) return IEM_OK;
  if (mode == 1) {
    DevGuard dg_(k->m->device);
    int rc = kkt_border_setup(k->m);
    if (rc) return rc;
  }
  k->border_mode = mode;
  k->factored = false;
  return IEM_OK;
}

int iem_kkt_factor_async(iem_kkt *k, int64_t *d_inertia) {
  if (!k || !d_inertia) return fail(IEM_E_ARG, "null argument");
  const iem::KktLayout &L = k->L;
  if (L.hubs) return fail(IEM_E_ARG, "iem_kkt_factor_async: hub mode factorises with host steps between its launches (iem_kkt_factor)");
  if (L.ne > 0 && k->border_mode != 1) return fail(IEM_E_ARG, "iem_kkt_factor_async: the border is factorised on the host in mode 0 (iem_kkt_set_border(k, 1) first)");
  iem_model *m = k->m;
  DevGuard dg_(m->device);
  int rc = kkt_border_setup(m);
  if (rc || (rc = kkt_factor_launch(k))) return rc;
  struct { const long long *info; long long *out; long long n; } A{k->d_info, (long long *)d_inertia, (long long)(L.nvar + L.ncon)};
  if ((rc = kkt_launch_raw(m, m->fixed[F_KBORDER].fn[KBORDER_INERTIA], &A, sizeof A, 1, 64))) return rc;
  k->factored = true;
  return IEM_OK;
}

int iem_kkt_factor(iem_kkt *k, int64_t *out_inertia) {
  if (!k) return fail(IEM_E_ARG, "null argument");
  iem_model *m = k->m;
  DevGuard dg_(m->device);
  const iem::KktLayout &L = k->L;
  if (L.hubs) return hub_factor(k, out_inertia);
  int rc = kkt_factor_launch(k);
  if (rc) return rc;
  int64_t neg = 0, doubtful = 0;
  if (L.ne > 0 && k->border_mode == 0) {      // the border: G - sum_k Gp[k] on the host (ne <= 64)
    std::vector<double> gp, G((size_t)(L.ne * L.ne));
    if ((rc = kkt_colsum_host(k, k->d_Gp, L.S, (int64_t)L.ne * L.ne, gp))) return rc;
    HIP_TRY(hipMemcpy(G.data(), k->d_flat + L.oG(), G.size() * 8, hipMemcpyDeviceToHost));
    k->Gs.resize(G.size());
    for (size_t i = 0; i < G.size(); ++i) k->Gs[i] = G[i] - gp[i];
    if (L.ne <= 64) {
      std::vector<double> ev;
      iem::sym_eigenvalues(k->Gs, L.ne, ev);
      double emax = 0.0;
      for (double e : ev) emax = std::max(emax, std::fabs(e));
      for (double e : ev) {
        // a zero / near-zero eigenvalue is neither sign: reported as DOUBTFUL so that a host doing the usual inertia correction
        // (neg == ncon && doubtful == 0) shifts and factorises again instead of solving with a singular border
        if (std::fabs(e) <= 1e-14 * emax || emax == 0.0) ++doubtful;
        else if (e < 0.0) ++neg;
      }
    } else {      // (a laned 2-D grid's border, up to 128: LDL' pivot signs instead of Jacobi sweeps)
      int64_t bn = 0, bd = 0;
      iem::sym_inertia_ldl(k->Gs, L.ne, bn, bd);
      // the padding's unit diagonal (n_border .. ne) is positive: nothing to subtract
      neg += bn; doubtful += bd;
    }
  }
  long long info[3] = {0, 0, 0};
  HIP_TRY(hipStreamSynchronize(m->stream));
  HIP_TRY(hipMemcpy(info, k->d_info, 24, hipMemcpyDeviceToHost));
  neg += info[0]; doubtful += info[1];
  k->factored = true;
  if (out_inertia) { out_inertia[0] = L.nvar + L.ncon - neg; out_inertia[1] = neg; out_inertia[2] = doubtful; }
  return IEM_OK;
}

/* ---- solve, residual and refined solve of the object: ONE implementation each, over nrhs columns (nrhs = 1, ld = nvar + ncon, no
 * per-row diagonal: the single-column entry points).  An entry point makes its refusals in its own name (`who`), then calls the
 * implementation.  K = [W + diag(sigma) + delta_w I, J'; J, -diag(dcon + delta_c)]  (csrc/iem_kkt_diag_device.h) ---------------------- */
namespace {
constexpr int KKT_DIAG_SLAB = 8;      // columns per pass of a residual / a refined solve: a multiple of every chunk width of the multi-column kernels (kkt_many_width: 2 or 4)
long long kkt_stream_grid(int64_t n) { return (long long)std::min<int64_t>((n + 255) / 256, 4096); }
// the whole extent [d, d + (nrhs - 1) ld + n) of a set of columns
int64_t kkt_extent(int nrhs, int64_t ld, int64_t n) { return (int64_t)(nrhs - 1) * ld + n; }
int kkt_refuse(const char *who, const char *what) { return fail(IEM_E_ARG, std::string(who) + ": " + what); }
// what every call over columns refuses first (nrhs before the object is looked at)
int kkt_columns_refusals(const char *who, const iem_kkt *k, int nrhs, std::initializer_list<const void *> vectors, std::initializer_list<int64_t> lds) {
  if (!k) return kkt_refuse(who, "null argument");
  for (const void *v : vectors) if (!v) return kkt_refuse(who, "null argument");
  if (nrhs < 1) return kkt_refuse(who, "nrhs must be at least 1");
  for (int64_t ld : lds) if (ld < k->L.nvar + k->L.ncon) return kkt_refuse(who, "a leading dimension is shorter than nvar + ncon");
  return IEM_OK;
}
const char *kNoFactorisation = "iem_kkt_solve: no factorisation (iem_kkt_assemble + iem_kkt_factor first)";      // (one sentence, whoever refuses)

int kkt_solve_refusals(const char *who, const iem_kkt *k, int nrhs, const double *d_rhs, int64_t ld_rhs, const double *d_sol, int64_t ld_sol) {
  int rc = kkt_columns_refusals(who, k, nrhs, {d_rhs, d_sol}, {ld_rhs, ld_sol});
  if (rc) return rc;
  const int64_t n = k->L.nvar + k->L.ncon;
  // in place column for column, or apart.  (Address ranges as integers: the two may be unrelated allocations.  Whole extents are
  // compared — columns of one array interleaved with columns of the other are refused too)
  if (!(d_sol == d_rhs && ld_sol == ld_rhs) && kkt_overlap(d_rhs, kkt_extent(nrhs, ld_rhs, n), d_sol, kkt_extent(nrhs, ld_sol, n)))
    return kkt_refuse(who, "d_rhs and d_sol overlap (allowed: the same array with the same leading dimension)");
  if (!k->factored) return fail(IEM_E_ARG, kNoFactorisation);
  return IEM_OK;
}
// the solve behind those refusals: chunks of the shape's width (a chunk of ONE column runs the single-column kernels of the chain)
int kkt_solve_columns(iem_kkt *k, int nrhs, const double *d_rhs, int64_t ld_rhs, double *d_sol, int64_t ld_sol) {
  const iem::KktLayout &L = k->L;
  iem_model *m = k->m;
  DevGuard dg_(m->device);
  int rc;
  if (L.hubs) {      // the hubs' side is GEMV work per column (hub_solve): a loop — sharing the hubs' factors across columns is not done here
    for (int u = 0; u < nrhs; ++u)
      if ((rc = hub_solve(k, d_rhs + (int64_t)u * ld_rhs, d_sol + (int64_t)u * ld_sol))) return rc;
    return IEM_OK;
  }
  const int R = k->km->many_r;
  const int64_t pl = L.S * L.nb, ne = L.ne, wp = 513 * std::max<int64_t>(ne, 1);      // wp: per column 512 partial rows of the column sums + the result, in d_part
  if ((rc = kkt_chunk_workspace(k, nrhs > 1 ? R : 1))) return rc;      // (one column: what iem_kkt_create allocated)
  double *w_r = k->w_r, *w_z = k->w_z, *w_rBp = k->w_rBp, *w_xB = k->w_xB;
  const bool chained = L.reach > 0;
  const double *Dinv = k->d_flat + L.oD(), *Bt = k->d_flat + L.oB();
  struct Mv { double *dst; const double *src; const long long *di, *si; long long n, ldd, lds; int nr; };
  auto move = [&](Mv A, int64_t cnt) { A.n = (long long)cnt; return kkt_launch_raw(m, k->km->move_m, &A, sizeof A, (cnt + 255) / 256, 256); };
  auto chain = [&](int nr, int phase) {
    return iem_kkt_chain_solve_many(m, L.S, L.S, L.nb, L.ne, L.nc, Dinv, chained ? Bt : nullptr, chained ? k->d_BR : nullptr, chained ? k->d_rows : nullptr,
                                    chained ? k->d_cols : nullptr, k->d_Z, w_r, chained ? w_z : nullptr, w_rBp, (phase && ne > 0) ? w_xB : nullptr, nr, phase);
  };
  std::vector<double> rB, col;
  for (int c0 = 0; c0 < nrhs; c0 += R) {
    const int nr = std::min(R, nrhs - c0);
    const double *rhs = d_rhs + (int64_t)c0 * ld_rhs;
    double *sol = d_sol + (int64_t)c0 * ld_sol;
    HIP_TRY(hipMemsetAsync(w_r, 0, (size_t)(nr * pl) * 8, m->stream));
    if ((rc = move(Mv{w_r, rhs, k->d_pos, k->d_on, 0, (long long)pl, (long long)ld_rhs, nr}, k->n_on))) return rc;
    if ((rc = chain(nr, 0))) return rc;
    if (ne > 0 && k->border_mode == 1) {      // the border systems on the device: ONE launch, a workgroup per column
      if ((rc = kkt_border_sums(m, k->km->colsum_m, w_rBp, (long long)(L.S * ne), L.S, ne, nr, k->d_part, (long long)wp, 512LL * ne))) return rc;
      if ((rc = kkt_border_solve_run(m, KktBorderSolveArgsH{k->d_F, k->d_piv, rhs, k->d_border, k->d_bloc, k->d_part + 512 * ne, w_xB, (long long)ld_rhs, (long long)wp,
                                                            (long long)ne, (int)ne, (int)L.n_border}, nr)))
        return rc;
    } else if (ne > 0) {      // the border systems on the host: Gs xB = rB - sum_k rBp[k] per column — ONE read-back and ONE upload per chunk
      if ((rc = kkt_border_sums(m, k->km->colsum_m, w_rBp, (long long)(L.S * ne), L.S, ne, nr, k->d_part, (long long)wp, 512LL * ne))) return rc;
      if (L.n_border) {
        HIP_TRY(hipMemsetAsync(w_xB, 0, (size_t)(nr * ne) * 8, m->stream));
        if ((rc = move(Mv{w_xB, rhs, k->d_bloc, k->d_border, 0, (long long)ne, (long long)ld_rhs, nr}, L.n_border))) return rc;
      }
      rB.assign((size_t)(nr * ne), 0.0);
      std::vector<double> rbp((size_t)(nr * ne));
      HIP_TRY(hipStreamSynchronize(m->stream));
      HIP_TRY(hipMemcpy2D(rbp.data(), (size_t)ne * 8, k->d_part + 512 * ne, (size_t)wp * 8, (size_t)ne * 8, (size_t)nr, hipMemcpyDeviceToHost));
      if (L.n_border) HIP_TRY(hipMemcpy(rB.data(), w_xB, (size_t)(nr * ne) * 8, hipMemcpyDeviceToHost));
      for (int u = 0; u < nr; ++u) {
        col.assign((size_t)ne, 0.0);
        for (int i = 0; i < ne; ++i) col[(size_t)i] = (i < L.n_border ? rB[(size_t)(u * ne + i)] : 0.0) - rbp[(size_t)(u * ne + i)];
        if (!iem::dense_solve(k->Gs, L.ne, col)) return fail(IEM_E_ARG, "iem_kkt_solve: the border's Schur complement is singular");
        std::copy(col.begin(), col.end(), rB.begin() + (size_t)u * (size_t)ne);
      }
      HIP_TRY(hipMemcpyAsync(w_xB, rB.data(), (size_t)(nr * ne) * 8, hipMemcpyHostToDevice, m->stream));
      HIP_TRY(hipStreamSynchronize(m->stream));      // (rB is a host temporary)
    }
    if ((rc = chain(nr, 1))) return rc;
    if ((rc = move(Mv{sol, w_r, k->d_on, k->d_pos, 0, (long long)ld_sol, (long long)pl, nr}, k->n_on))) return rc;
    if (L.n_border && (rc = move(Mv{sol, w_xB, k->d_border, k->d_bloc, 0, (long long)ld_sol, (long long)ne, nr}, L.n_border))) return rc;
  }
  return IEM_OK;
}

// the planes p | r | dsol for `nrhs` columns (one column, or one slab): the synchronous part of the first residual or refined call,
// grown like the solves' workspace
int kkt_refine_workspace(iem_kkt *k, int nrhs) {
  const int cols = nrhs > 1 ? KKT_DIAG_SLAB : 1;
  if (k->ref_cols >= cols) return IEM_OK;
  if (k->w_ref) { HIP_TRY(hipStreamSynchronize(k->m->stream)); hipFree(k->w_ref); k->w_ref = nullptr; k->ref_cols = 0; }
  HIP_TRY(hipMalloc((void **)&k->w_ref, (size_t)std::max<int64_t>(3 * cols * (k->L.nvar + k->L.ncon), 1) * 8));
  k->ref_cols = cols;
  return IEM_OK;
}
// the residuals of nr <= ref_cols columns: one iem_kktprod per column into the p planes, then ONE launch
int kkt_residual_slab(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma, const double *d_dcon, double delta_w, double delta_c,
                      int nr, const double *d_rhs, int64_t ld_rhs, const double *d_sol, int64_t ld_sol, double *d_r, int64_t ld_r, double *d_norms) {
  iem_model *m = k->m;
  const int64_t nvar = k->L.nvar, ncon = k->L.ncon, n = nvar + ncon;
  double *p = k->w_ref;
  int rc;
  for (int u = 0; u < nr; ++u) {
    const double *s = d_sol + (int64_t)u * ld_sol;
    double *pu = p + (int64_t)u * n;
    if ((rc = iem_kktprod(m, d_x, d_y, obj_weight, s, ncon ? s + nvar : nullptr, pu, ncon ? pu + nvar : nullptr))) return rc;
  }
  if (d_norms) HIP_TRY(hipMemsetAsync(d_norms, 0, (size_t)nr * 8, m->stream));
  struct { const double *p, *rhs, *sol, *sigma, *dcon; double *r; unsigned long long *norms; double dw, dc; long long nvar, n, ld_p, ld_rhs, ld_sol, ld_r; } A{
      p, d_rhs, d_sol, d_sigma, ncon ? d_dcon : nullptr, d_r, (unsigned long long *)d_norms, delta_w, delta_c, (long long)nvar, (long long)n, (long long)n,
      (long long)ld_rhs, (long long)ld_sol, (long long)ld_r};
  return kkt_launch_raw(m, m->fixed[F_KDIAG].fn[KDIAG_RESIDUAL], &A, sizeof A, kkt_stream_grid(n), 256, nr);
}

int kkt_residual_refusals(const char *who, const iem_kkt *k, int nrhs, const double *d_rhs, int64_t ld_rhs, const double *d_sol, int64_t ld_sol, const double *d_r,
                          int64_t ld_r, const double *d_norms) {
  int rc = kkt_columns_refusals(who, k, nrhs, {d_rhs, d_sol, d_r}, {ld_rhs, ld_sol, ld_r});
  if (rc) return rc;
  const int64_t n = k->L.nvar + k->L.ncon, er = kkt_extent(nrhs, ld_r, n), eb = kkt_extent(nrhs, ld_rhs, n), es = kkt_extent(nrhs, ld_sol, n);
  if (kkt_overlap(d_r, er, d_sol, es) || (!(d_r == d_rhs && ld_r == ld_rhs) && kkt_overlap(d_r, er, d_rhs, eb)) || kkt_overlap(d_r, er, d_norms, nrhs) ||
      kkt_overlap(d_norms, nrhs, d_sol, es) || kkt_overlap(d_norms, nrhs, d_rhs, eb))
    return kkt_refuse(who, "overlap — d_r overlaps d_sol or d_rhs (allowed: d_r == d_rhs with the same leading dimension), or d_norms lies inside the vectors");
  return IEM_OK;
}
int kkt_residual_columns(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma, const double *d_dcon, double delta_w, double delta_c,
                         int nrhs, const double *d_rhs, int64_t ld_rhs, const double *d_sol, int64_t ld_sol, double *d_r, int64_t ld_r, double *d_norms) {
  DevGuard dg_(k->m->device);
  int rc = kkt_refine_workspace(k, nrhs);
  if (rc) return rc;
  for (int c0 = 0; c0 < nrhs; c0 += KKT_DIAG_SLAB) {
    const int nr = std::min(KKT_DIAG_SLAB, nrhs - c0);
    if ((rc = kkt_residual_slab(k, d_x, d_y, obj_weight, d_sigma, d_dcon, delta_w, delta_c, nr, d_rhs + (int64_t)c0 * ld_rhs, ld_rhs, d_sol + (int64_t)c0 * ld_sol, ld_sol,
                                d_r + (int64_t)c0 * ld_r, ld_r, d_norms ? d_norms + c0 : nullptr)))
      return rc;
  }
  return IEM_OK;
}

int kkt_refined_refusals(const char *who, const iem_kkt *k, int nrhs, const double *d_rhs, int64_t ld_rhs, const double *d_sol, int64_t ld_sol, int steps,
                         const double *d_norms) {
  int rc = kkt_columns_refusals(who, k, nrhs, {d_rhs, d_sol}, {ld_rhs, ld_sol});
  if (rc) return rc;
  if (steps < 0) return kkt_refuse(who, "steps must not be negative");
  const int64_t n = k->L.nvar + k->L.ncon, eb = kkt_extent(nrhs, ld_rhs, n), es = kkt_extent(nrhs, ld_sol, n), en = (int64_t)(steps + 1) * nrhs;
  if (kkt_overlap(d_sol, es, d_rhs, eb) || kkt_overlap(d_norms, en, d_sol, es) || kkt_overlap(d_norms, en, d_rhs, eb))
    return kkt_refuse(who, "overlap — d_sol, d_rhs and d_norms may not overlap");
  if (!k->factored) return fail(IEM_E_ARG, kNoFactorisation);
  return IEM_OK;
}
// solve, then `steps` times residual, solve of it, add; the norms in front of every step and behind the last
int kkt_refined_columns(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma, const double *d_dcon, double delta_w, double delta_c,
                        int nrhs, const double *d_rhs, int64_t ld_rhs, double *d_sol, int64_t ld_sol, int steps, double *d_norms) {
  iem_model *m = k->m;
  DevGuard dg_(m->device);
  int rc = kkt_refine_workspace(k, nrhs);
  if (rc) return rc;
  const int64_t n = k->L.nvar + k->L.ncon;
  double *r = k->w_ref + (int64_t)k->ref_cols * n, *dsol = k->w_ref + 2 * (int64_t)k->ref_cols * n;
  // slab by slab (the columns do not interact, and the chunks of the solve inside a slab are those of the whole set)
  for (int c0 = 0; c0 < nrhs; c0 += KKT_DIAG_SLAB) {
    const int nr = std::min(KKT_DIAG_SLAB, nrhs - c0);
    const double *rhs = d_rhs + (int64_t)c0 * ld_rhs;
    double *sol = d_sol + (int64_t)c0 * ld_sol;
    auto residual = [&](int i) {
      return kkt_residual_slab(k, d_x, d_y, obj_weight, d_sigma, d_dcon, delta_w, delta_c, nr, rhs, ld_rhs, sol, ld_sol, r, n, d_norms ? d_norms + (int64_t)i * nrhs + c0 : nullptr);
    };
    if ((rc = kkt_solve_columns(k, nr, rhs, ld_rhs, sol, ld_sol))) return rc;
    for (int i = 0; i < steps; ++i) {
      if ((rc = residual(i))) return rc;
      if ((rc = kkt_solve_columns(k, nr, r, n, dsol, n))) return rc;
      struct { double *sol; const double *d; long long n, ld_s, ld_d; } A{sol, dsol, (long long)n, (long long)ld_sol, (long long)n};
      if ((rc = kkt_launch_raw(m, m->fixed[F_KDIAG].fn[KDIAG_AXPY], &A, sizeof A, kkt_stream_grid(n), 256, nr))) return rc;
    }
    if (d_norms && (rc = residual(steps))) return rc;
  }
  return IEM_OK;
}
}  // namespace

int iem_kkt_diag_source(char **out_src, uint64_t *out_key) { return fixed_source_out(F_KDIAG, out_src, out_key); }

int iem_kkt_solve(iem_kkt *k, const double *d_rhs, double *d_sol) {
  const int64_t n = k ? k->L.nvar + k->L.ncon : 0;
  int rc = kkt_solve_refusals("iem_kkt_solve", k, 1, d_rhs, n, d_sol, n);
  return rc ? rc : kkt_solve_columns(k, 1, d_rhs, n, d_sol, n);
}

int iem_kkt_solve_many(iem_kkt *k, int nrhs, const double *d_rhs, int64_t ld_rhs, double *d_sol, int64_t ld_sol) {
  int rc = kkt_solve_refusals("iem_kkt_solve_many", k, nrhs, d_rhs, ld_rhs, d_sol, ld_sol);
  return rc ? rc : kkt_solve_columns(k, nrhs, d_rhs, ld_rhs, d_sol, ld_sol);
}

int iem_kkt_residual(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma, double delta_w, double delta_c,
                     const double *d_rhs, const double *d_sol, double *d_r, double *d_norm) {
  const int64_t n = k ? k->L.nvar + k->L.ncon : 0;
  int rc = kkt_residual_refusals("iem_kkt_residual", k, 1, d_rhs, n, d_sol, n, d_r, n, d_norm);
  return rc ? rc : kkt_residual_columns(k, d_x, d_y, obj_weight, d_sigma, nullptr, delta_w, delta_c, 1, d_rhs, n, d_sol, n, d_r, n, d_norm);
}

int iem_kkt_solve_refined(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma, double delta_w, double delta_c,
                          const double *d_rhs, double *d_sol, int steps, double *d_norms) {
  const int64_t n = k ? k->L.nvar + k->L.ncon : 0;
  int rc = kkt_refined_refusals("iem_kkt_solve_refined", k, 1, d_rhs, n, d_sol, n, steps, d_norms);
  return rc ? rc : kkt_refined_columns(k, d_x, d_y, obj_weight, d_sigma, nullptr, delta_w, delta_c, 1, d_rhs, n, d_sol, n, steps, d_norms);
}

int iem_kkt_assemble_diag(iem_kkt *k, const double *d_hess, const double *d_jac, const double *d_sigma, const double *d_dcon, double delta_w, double delta_c) {
  if (!k || (!d_hess && k->n_h) || (!d_jac && k->n_j)) return fail(IEM_E_ARG, "null argument");
  iem_model *m = k->m;
  DevGuard dg_(m->device);
  const iem::KktLayout &L = k->L;
  HIP_TRY(hipMemsetAsync(k->d_flat, 0, (size_t)L.total() * 8, m->stream));
  struct { double *flat; const long long *dest; const unsigned *seg, *perm; const double *hess, *jac, *sigma, *dcon; double dw, dc; long long n_dest, n_h, n_j, n_var, n_con; } A{
      k->d_flat, k->d_dest, k->d_seg, k->d_perm, d_hess, d_jac, d_sigma, d_dcon, delta_w, delta_c, (long long)k->n_dest, (long long)k->n_h, (long long)k->n_j,
      (long long)L.nvar, (long long)L.ncon};
  k->factored = false;
  return kkt_launch_raw(m, m->fixed[F_KDIAG].fn[KDIAG_GATHER], &A, sizeof A, (k->n_dest + 255) / 256, 256);
}

int iem_kkt_residual_diag(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma, const double *d_dcon, double delta_w,
                          double delta_c, int nrhs, const double *d_rhs, int64_t ld_rhs, const double *d_sol, int64_t ld_sol, double *d_r, int64_t ld_r, double *d_norms) {
  int rc = kkt_residual_refusals("iem_kkt_residual_diag", k, nrhs, d_rhs, ld_rhs, d_sol, ld_sol, d_r, ld_r, d_norms);
  return rc ? rc : kkt_residual_columns(k, d_x, d_y, obj_weight, d_sigma, d_dcon, delta_w, delta_c, nrhs, d_rhs, ld_rhs, d_sol, ld_sol, d_r, ld_r, d_norms);
}

int iem_kkt_solve_refined_diag(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma, const double *d_dcon, double delta_w,
                               double delta_c, int nrhs, const double *d_rhs, int64_t ld_rhs, double *d_sol, int64_t ld_sol, int steps, double *d_norms) {
  int rc = kkt_refined_refusals("iem_kkt_solve_refined_diag", k, nrhs, d_rhs, ld_rhs, d_sol, ld_sol, steps, d_norms);
  return rc ? rc : kkt_refined_columns(k, d_x, d_y, obj_weight, d_sigma, d_dcon, delta_w, delta_c, nrhs, d_rhs, ld_rhs, d_sol, ld_sol, steps, d_norms);
}

/* ---- the interior-point barrier layer: what sits between the evaluation calls and the KKT object (csrc/iem_barrier_device.h) ---- */
struct iem_barrier {
  iem_model *m = nullptr;
  int64_t nvar = 0, ncon = 0, n_eq = 0, n_ineq = 0, n_xl = 0, n_xu = 0, n_sl = 0, n_su = 0, n_wg = 0;
  double *d_bounds = nullptr;          // xl | xu (nvar each) | rl | ru | ceq (ncon each)
  unsigned char *d_flags = nullptr;    // fx (nvar) | fc (ncon)
  double *d_red = nullptr;             // 4 n_wg parked values + the ticket words (zeroed once; the tickets reset themselves)
  long long *d_tab = nullptr;          // offs[4] | first[4] | count[4] of iem_shared_totals
  unsigned long long *d_ones = nullptr;   // the bits of {1.0, 1.0}: what the step lengths are seeded with (device-to-device copy)
  const double *mu_blk = nullptr;      // iem_barrier_bind_mu: the block of an iem_mu object (borrowed), or null
};

namespace {
// BarrierArgs of csrc/iem_barrier_device.h
struct BarrierArgsH {
  const double *xl, *xu, *rl, *ru, *ceq;
  const unsigned char *fx, *fc;
  double *x, *s, *y, *zL, *zU, *vL, *vU;
  const double *r, *c, *sol;
  double *ds, *dzL, *dzU, *dvL, *dvU;
  double *sigma, *dcon, *rhs;
  unsigned long long *alpha;
  double *out;
  double *red;
  const long long *tab;
  double mu, tau, kappa, push, frac;
  long long nvar, n, n_wg;
  const double *mu_blk;
};
BarrierArgsH barrier_args(const iem_barrier *b) {
  BarrierArgsH A;
  std::memset(&A, 0, sizeof A);
  A.xl = b->d_bounds; A.xu = A.xl + b->nvar; A.rl = A.xu + b->nvar; A.ru = A.rl + b->ncon; A.ceq = A.ru + b->ncon;
  A.fx = b->d_flags; A.fc = A.fx + b->nvar;
  A.red = b->d_red; A.tab = b->d_tab;
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon); A.n_wg = (long long)b->n_wg;
  A.mu_blk = b->mu_blk;
  return A;
}
// unbound: the barrier object as it always was (its BarrierArgs ends in front of mu_blk); bound: the variant below, which reads the block
int barrier_launch(const iem_barrier *b, int which, BarrierArgsH &A) {
  if (A.mu_blk) return kkt_launch_raw(b->m, b->m->barrier_mu.fn[which], &A, sizeof A, b->n_wg, 256);
  return kkt_launch_raw(b->m, b->m->fixed[F_BARRIER].fn[which], &A, offsetof(BarrierArgsH, mu_blk), b->n_wg, 256);
}
// The BOUND variant of the barrier code object: the text of csrc/iem_barrier_device.h with BarrierArgs one pointer longer and the single
// read of mu (barrier_step: and of tau) in barrier_terms / step / update / error taken from the block — derived from the one text, so
// that the unbound object keeps its source, its key and its bits, and the two cannot drift apart.  Every pattern must match exactly as
// often as listed: an edit of the header that breaks one is an error here, not a silently unbound kernel.
int barrier_mu_source(std::string &s) {
  static const struct { const char *from, *to; int times; } kEdits[] = {
      {"  long long nvar, n, n_wg;\n};", "  long long nvar, n, n_wg;\n  const double *mu_blk;      // the iem_mu block {mu, tau, ...}\n};", 1},
      {"  const double mu = A.mu;\n", "  const double mu = A.mu_blk[0];\n", 2},      // barrier_terms, barrier_error
      {"  const double mu = A.mu, tau = A.tau, ntau = -A.tau;\n", "  const double mu = A.mu_blk[0], tau = A.mu_blk[1], ntau = -tau;\n", 1},      // barrier_step
      {"  const double mu = A.mu, kappa = A.kappa;\n", "  const double mu = A.mu_blk[0], kappa = A.kappa;\n", 1},      // barrier_update
  };
  std::string text(kBarrierSource);
  for (const auto &e : kEdits) {
    const std::string from(e.from), to(e.to);
    int seen = 0;
    for (size_t at = text.find(from); at != std::string::npos; at = text.find(from, at + to.size())) {
      text.replace(at, from.size(), to);
      ++seen;
    }
    if (seen != e.times) return fail(IEM_E_COMPILE, std::string("internal: the barrier kernels do not read mu where the bound variant expects it: ") + e.from);
  }
  return object_source(text.c_str(), true, s);
}
int barrier_mu_object(iem_model *m) {
  iem_model::FixedObject &o = m->barrier_mu;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = barrier_mu_source(src);
  if (rc) return rc;
  KernelSlot slots[kFixedSlots];
  int n = 0;
  for (; n < kFixedSlots && kFixed[F_BARRIER].kernels[n]; ++n) slots[n] = KernelSlot{kFixed[F_BARRIER].kernels[n], &o.fn[n]};
  return load_object(m, src, slots, n, &o.mod);
}
// the state vectors a call needs: x with variables, y and the slack side with rows (the slack side only with inequality rows)
bool barrier_state_missing(const iem_barrier *b, const double *x, const double *s, const double *y, const double *zL, const double *zU, const double *vL, const double *vU) {
  return (b->nvar && (!x || !zL || !zU)) || (b->ncon && !y) || (b->n_ineq && (!s || !vL || !vU));
}
// the host analysis of iem_barrier_create: relaxed bounds xl | xu | rl | ru | ceq, flags fx | fc, counts — and its refusals
int barrier_analyse(int64_t nvar, int64_t ncon, const double *const src[4], double relax, double *bounds, unsigned char *flags, iem_barrier *hb) {
  if (!(relax >= 0.0) || !std::isfinite(relax)) return fail(IEM_E_ARG, "iem_barrier_create: relax must be finite and not negative");
  const double inf = std::numeric_limits<double>::infinity();
  auto lo = [&](double v) { return std::isfinite(v) ? v - relax * std::max(1.0, std::fabs(v)) : -inf; };
  auto hi = [&](double v) { return std::isfinite(v) ? v + relax * std::max(1.0, std::fabs(v)) : inf; };
  hb->nvar = nvar; hb->ncon = ncon;
  hb->n_eq = hb->n_ineq = hb->n_xl = hb->n_xu = hb->n_sl = hb->n_su = 0;
  double *xl = bounds, *xu = xl + nvar, *rl = xu + nvar, *ru = rl + ncon, *ceq = ru + ncon;
  for (int64_t i = 0; i < nvar; ++i) {
    const double l = src[0][i], u = src[1][i];
    if (l != l || u != u || l > u || l == inf || u == -inf) return fail(IEM_E_ARG, "iem_barrier_create: variable " + std::to_string(i) + " has lvar > uvar (or a NaN / an infinite bound of the wrong sign)");
    if (l == u && relax == 0.0) return fail(IEM_E_ARG, "iem_barrier_create: variable " + std::to_string(i) + " is fixed (lvar == uvar) and relax is 0: it has no interior");
    xl[i] = lo(l); xu[i] = hi(u);
    flags[(size_t)i] = (unsigned char)((std::isfinite(l) ? 1 : 0) | (std::isfinite(u) ? 2 : 0));
    hb->n_xl += std::isfinite(l); hb->n_xu += std::isfinite(u);
  }
  for (int64_t j = 0; j < ncon; ++j) {
    const double l = src[2][j], u = src[3][j];
    if (l != l || u != u || l > u || l == inf || u == -inf) return fail(IEM_E_ARG, "iem_barrier_create: row " + std::to_string(j) + " has lcon > ucon (or a NaN / an infinite bound of the wrong sign)");
    if (!std::isfinite(l) && !std::isfinite(u)) return fail(IEM_E_ARG, "iem_barrier_create: row " + std::to_string(j) + " has neither bound (a free row has no slack to eliminate)");
    if (l == u) {
      rl[j] = -inf; ru[j] = inf; ceq[j] = l;
      flags[(size_t)(nvar + j)] = 4;
      ++hb->n_eq;
    } else {
      rl[j] = lo(l); ru[j] = hi(u); ceq[j] = 0.0;
      flags[(size_t)(nvar + j)] = (unsigned char)((std::isfinite(l) ? 1 : 0) | (std::isfinite(u) ? 2 : 0));
      hb->n_sl += std::isfinite(l); hb->n_su += std::isfinite(u);
      ++hb->n_ineq;
    }
  }
  hb->n_wg = std::max<long long>(kkt_stream_grid(nvar + ncon), 1);
  return IEM_OK;
}
int barrier_info_out(const iem_barrier *b, iem_barrier_info_t *out) {
  if (out->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_barrier_info: set struct_size to sizeof(iem_barrier_info_t) before the call");
  iem_barrier_info_t v;
  v.struct_size = std::min<uint64_t>(out->struct_size, sizeof v);
  v.nvar = b->nvar; v.ncon = b->ncon; v.n_eq = b->n_eq; v.n_ineq = b->n_ineq;
  v.n_xl = b->n_xl; v.n_xu = b->n_xu; v.n_sl = b->n_sl; v.n_su = b->n_su;
  v.nz = b->n_xl + b->n_xu + b->n_sl + b->n_su;
  v.workgroups = b->n_wg;
  std::memcpy(out, &v, (size_t)v.struct_size);      // never more than the caller's struct holds
  return IEM_OK;
}
}  // namespace

int iem_barrier_analyse(int64_t nvar, int64_t ncon, const double *h_lvar, const double *h_uvar, const double *h_lcon, const double *h_ucon, double relax,
                        double *h_bounds, uint8_t *h_flags, iem_barrier_info_t *info) {
  if (nvar < 0 || ncon < 0 || (nvar && (!h_lvar || !h_uvar)) || (ncon && (!h_lcon || !h_ucon)) || !h_bounds || !h_flags || !info) return fail(IEM_E_ARG, "null argument");
  const double *src[4] = {h_lvar, h_uvar, h_lcon, h_ucon};
  iem_barrier hb;
  int rc = barrier_analyse(nvar, ncon, src, relax, h_bounds, h_flags, &hb);
  return rc ? rc : barrier_info_out(&hb, info);
}

int iem_barrier_source(char **out_src, uint64_t *out_key) { return fixed_source_out(F_BARRIER, out_src, out_key); }

int iem_barrier_destroy(iem_barrier *b) {
  if (!b) return IEM_OK;
  DevGuard dg_(b->m->device);
  for (void *p : {(void *)b->d_bounds, (void *)b->d_flags, (void *)b->d_red, (void *)b->d_tab, (void *)b->d_ones})
    if (p) hipFree(p);
  delete b;
  return IEM_OK;
}

int iem_barrier_create(iem_model *m, const double *h_lvar, const double *h_uvar, const double *h_lcon, const double *h_ucon, double relax, iem_barrier **out) {
  if (!m || !out) return fail(IEM_E_ARG, "null argument");
  if (m->sharded) return fail(IEM_E_ARG, "iem_barrier_create: a sharded handle holds one rank's window; the step lengths and error terms want the whole model");
  const int64_t nvar = m->model.nvar, ncon = m->model.ncon, n = nvar + ncon;
  std::vector<double> own[4];
  const double *src[4] = {h_lvar, h_uvar, h_lcon, h_ucon};
  static const int which[4] = {IEM_LVAR, IEM_UVAR, IEM_LCON, IEM_UCON};
  for (int a = 0; a < 4; ++a)
    if (!src[a]) {      // the handle's own host mirror
      own[a].resize((size_t)std::max<int64_t>(a < 2 ? nvar : ncon, 1));
      int rc = iem_get_host(m, which[a], own[a].data());
      if (rc) return rc;
      src[a] = own[a].data();
    }
  std::vector<double> bounds((size_t)std::max<int64_t>(2 * nvar + 3 * ncon, 1), 0.0);
  std::vector<unsigned char> flags((size_t)std::max<int64_t>(n, 1), 0);
  std::unique_ptr<iem_barrier> hb(new iem_barrier);
  hb->m = m;
  {
    int rc = barrier_analyse(nvar, ncon, src, relax, bounds.data(), flags.data(), hb.get());
    if (rc) return rc;
  }
  DevGuard dg_(m->device);
  {
    int rc = fixed_object(m, F_BARRIER);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_barrier *p) const { iem_barrier_destroy(p); } };      // (a failed create frees what it had uploaded)
  std::unique_ptr<iem_barrier, Drop> b(hb.release());
  const int64_t n_red = 4 * b->n_wg + 1 + (b->n_wg + 31) / 32;      // (IEM_TICKET_WORDS of csrc/iem_device.h)
  HIP_TRY(hipMalloc((void **)&b->d_bounds, bounds.size() * 8));
  HIP_TRY(hipMalloc((void **)&b->d_flags, flags.size()));
  HIP_TRY(hipMalloc((void **)&b->d_red, (size_t)n_red * 8));
  HIP_TRY(hipMalloc((void **)&b->d_tab, 12 * 8));
  HIP_TRY(hipMalloc((void **)&b->d_ones, 16));
  long long tab[12];
  for (int s = 0; s < 4; ++s) { tab[s] = s * (long long)b->n_wg; tab[4 + s] = 0; tab[8 + s] = (long long)b->n_wg; }
  const double ones[2] = {1.0, 1.0};
  HIP_TRY(hipMemcpy(b->d_bounds, bounds.data(), bounds.size() * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_flags, flags.data(), flags.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(b->d_red, 0, (size_t)n_red * 8));
  HIP_TRY(hipMemcpy(b->d_tab, tab, sizeof tab, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_ones, ones, sizeof ones, hipMemcpyHostToDevice));
  *out = b.release();
  return IEM_OK;
}

int iem_barrier_info(const iem_barrier *b, iem_barrier_info_t *out) {
  if (!b || !out) return fail(IEM_E_ARG, "null argument");
  return barrier_info_out(b, out);
}

int iem_barrier_start(iem_barrier *b, double *d_x, const double *d_c, double *d_s, double *d_zL, double *d_zU, double *d_vL, double *d_vU, double bound_push,
                      double bound_frac) {
  if (!(bound_push > 0.0) || !(bound_frac > 0.0) || !(bound_frac <= 0.5) || !std::isfinite(bound_push))
    return fail(IEM_E_ARG, "iem_barrier_start: bound_push must be positive and bound_frac in (0, 0.5]");
  if (!b || barrier_state_missing(b, d_x, d_s, d_c, d_zL, d_zU, d_vL, d_vU) || (b->n_ineq && !d_c)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(b->m->device);
  BarrierArgsH A = barrier_args(b);
  A.x = d_x; A.c = d_c; A.s = d_s; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU; A.push = bound_push; A.frac = bound_frac;
  return barrier_launch(b, BAR_START, A);
}

int iem_barrier_terms(iem_barrier *b, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                      const double *d_vU, const double *d_r, const double *d_c, double mu, double *d_sigma, double *d_dcon, double *d_rhs) {
  if (!(b && b->mu_blk) && !(mu >= 0.0)) return fail(IEM_E_ARG, "iem_barrier_terms: mu must not be negative");
  if (!b || barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || (b->nvar && (!d_r || !d_sigma)) || (b->ncon && (!d_c || !d_dcon)) || !d_rhs)
    return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(b->m->device);
  BarrierArgsH A = barrier_args(b);
  A.x = (double *)d_x; A.s = (double *)d_s; A.y = (double *)d_y; A.zL = (double *)d_zL; A.zU = (double *)d_zU; A.vL = (double *)d_vL; A.vU = (double *)d_vU;
  A.r = d_r; A.c = d_c; A.mu = mu; A.sigma = d_sigma; A.dcon = d_dcon; A.rhs = d_rhs;
  return barrier_launch(b, BAR_TERMS, A);
}

int iem_barrier_step(iem_barrier *b, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                     const double *d_vU, const double *d_sol, double mu, double tau, double *d_ds, double *d_dzL, double *d_dzU, double *d_dvL, double *d_dvU,
                     double *d_alpha) {
  if (!(b && b->mu_blk) && !(mu >= 0.0)) return fail(IEM_E_ARG, "iem_barrier_step: mu must not be negative");
  if (!(b && b->mu_blk) && !(tau > 0.0 && tau <= 1.0)) return fail(IEM_E_ARG, "iem_barrier_step: tau must lie in (0, 1]");
  if (!b || barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || !d_sol || !d_alpha || (b->nvar && (!d_dzL || !d_dzU)) ||
      (b->n_ineq && (!d_ds || !d_dvL || !d_dvU)))
    return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  BarrierArgsH A = barrier_args(b);
  A.x = (double *)d_x; A.s = (double *)d_s; A.y = (double *)d_y; A.zL = (double *)d_zL; A.zU = (double *)d_zU; A.vL = (double *)d_vL; A.vU = (double *)d_vU;
  A.sol = d_sol; A.mu = mu; A.tau = tau; A.ds = d_ds; A.dzL = d_dzL; A.dzU = d_dzU; A.dvL = d_dvL; A.dvU = d_dvU; A.alpha = (unsigned long long *)d_alpha;
  // the seed: the bits of 1.0 (a memset cannot write that pattern; a device-to-device copy is a capturable node)
  HIP_TRY(hipMemcpyAsync(d_alpha, b->d_ones, 16, hipMemcpyDeviceToDevice, m->stream));
  return barrier_launch(b, BAR_STEP, A);
}

int iem_barrier_update(iem_barrier *b, double *d_x, double *d_s, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU, const double *d_sol,
                       const double *d_ds, const double *d_dzL, const double *d_dzU, const double *d_dvL, const double *d_dvU, const double *d_alpha, double mu,
                       double kappa_sigma) {
  if (!(b && b->mu_blk) && !(mu >= 0.0)) return fail(IEM_E_ARG, "iem_barrier_update: mu must not be negative");
  if (!(kappa_sigma >= 1.0)) return fail(IEM_E_ARG, "iem_barrier_update: kappa_sigma must be at least 1");
  if (!b || barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || !d_sol || !d_alpha || (b->nvar && (!d_dzL || !d_dzU)) ||
      (b->n_ineq && (!d_ds || !d_dvL || !d_dvU)))
    return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(b->m->device);
  BarrierArgsH A = barrier_args(b);
  A.x = d_x; A.s = d_s; A.y = d_y; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU;
  A.sol = d_sol; A.ds = (double *)d_ds; A.dzL = (double *)d_dzL; A.dzU = (double *)d_dzU; A.dvL = (double *)d_dvL; A.dvU = (double *)d_dvU;
  A.alpha = (unsigned long long *)d_alpha; A.mu = mu; A.kappa = kappa_sigma;
  return barrier_launch(b, BAR_UPDATE, A);
}

int iem_barrier_error(iem_barrier *b, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                      const double *d_vU, const double *d_r, const double *d_c, double mu, double *d_out) {
  if (!(b && b->mu_blk) && !(mu >= 0.0)) return fail(IEM_E_ARG, "iem_barrier_error: mu must not be negative");
  if (!b || barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || (b->ncon && !d_c) || !d_out) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  BarrierArgsH A = barrier_args(b);
  A.x = (double *)d_x; A.s = (double *)d_s; A.y = (double *)d_y; A.zL = (double *)d_zL; A.zU = (double *)d_zU; A.vL = (double *)d_vL; A.vU = (double *)d_vU;
  A.r = d_r; A.c = d_c; A.mu = mu; A.out = d_out;
  HIP_TRY(hipMemsetAsync(d_out, 0, 4 * 8, m->stream));      // the four maxima start from +0.0
  return barrier_launch(b, BAR_ERROR, A);
}

int iem_barrier_merit(iem_barrier *b, const double *d_x, const double *d_s, const double *d_c, double *d_out) {
  if (!b || (b->nvar && !d_x) || (b->n_ineq && !d_s) || (b->ncon && !d_c) || !d_out) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(b->m->device);
  BarrierArgsH A = barrier_args(b);
  A.x = (double *)d_x; A.s = (double *)d_s; A.c = d_c; A.out = d_out;
  return barrier_launch(b, BAR_MERIT, A);
}

/* ---- the filter line search: slope, trial point, acceptance (csrc/iem_search_device.h) ---- */
struct iem_search {
  iem_barrier *b = nullptr;
  iem_search_opts_t opt;
  double *d_ctl = nullptr;             // the control block: 16 words
  double *d_filter = nullptr;          // filter_capacity pairs (theta, phi)
  double *d_red = nullptr;             // n_wg parked values + the ticket words (zeroed once; the tickets reset themselves)
  long long *d_tab = nullptr;          // offs | first | count of iem_shared_totals
  const double *mu_blk = nullptr;      // iem_search_bind_mu: the block of an iem_mu object (borrowed), or null
};

namespace {
// SearchArgs of csrc/iem_search_device.h
struct SearchArgsH {
  const double *xl, *xu, *rl, *ru;
  const unsigned char *fx, *fc;
  const double *x, *s, *g, *sol, *ds;
  const double *obj, *err, *alpha_in;
  double *xt, *st;
  const double *ft, *merit;
  double *alpha_out;
  double *ctl, *filter;
  double *red;
  const long long *tab;
  double mu, sigma;
  double gamma_theta, gamma_phi, eta_phi, delta, s_theta, s_phi, alpha_floor;
  long long max_trials, capacity;
  long long nvar, n, n_wg;
  const double *mu_blk;
};
SearchArgsH search_args(const iem_search *s) {
  const iem_barrier *b = s->b;
  SearchArgsH A;
  std::memset(&A, 0, sizeof A);
  A.xl = b->d_bounds; A.xu = A.xl + b->nvar; A.rl = A.xu + b->nvar; A.ru = A.rl + b->ncon;
  A.fx = b->d_flags; A.fc = A.fx + b->nvar;
  A.ctl = s->d_ctl; A.filter = s->d_filter; A.red = s->d_red; A.tab = s->d_tab;
  A.gamma_theta = s->opt.gamma_theta; A.gamma_phi = s->opt.gamma_phi; A.eta_phi = s->opt.eta_phi; A.delta = s->opt.delta;
  A.s_theta = s->opt.s_theta; A.s_phi = s->opt.s_phi; A.alpha_floor = s->opt.alpha_floor;
  A.max_trials = (long long)s->opt.max_trials; A.capacity = (long long)s->opt.filter_capacity;
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon); A.n_wg = (long long)b->n_wg;
  A.mu_blk = s->mu_blk;
  return A;
}
const struct SearchSlot { const char *name; hipFunction_t iem_model::SearchObject::*fn; } kSearchSlots[] = {
    {"search_begin", &iem_model::SearchObject::begin},
    {"search_trial", &iem_model::SearchObject::trial},
    {"search_accept", &iem_model::SearchObject::accept},
};
int search_object(iem_model *m) {
  iem_model::SearchObject &o = m->search;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = object_source(kSearchSource, true, src);
  if (rc) return rc;
  KernelSlot slots[sizeof kSearchSlots / sizeof *kSearchSlots];
  int n = 0;
  for (const SearchSlot &ss : kSearchSlots) slots[n++] = KernelSlot{ss.name, &(o.*ss.fn)};
  return load_object(m, src, slots, n, &o.mod);
}
int search_opts(const iem_search_opts_t *in, iem_search_opts_t *out) {
  iem_search_opts_t v = {sizeof v, 1e-5, 1e-8, 1e-8, 1.0, 1.1, 2.3, 1e-16, 30, 64};      // Ipopt's
  if (in) {
    if (in->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_search_create: set struct_size to sizeof(iem_search_opts_t) before the call");
    std::memcpy(&v, in, (size_t)std::min<uint64_t>(in->struct_size, sizeof v));      // (fields a shorter struct does not have keep their defaults)
    v.struct_size = sizeof v;
  }
  auto unit = [](double g) { return g > 0.0 && g < 1.0; };
  if (!unit(v.gamma_theta) || !unit(v.gamma_phi) || !unit(v.eta_phi)) return fail(IEM_E_ARG, "iem_search_create: gamma_theta, gamma_phi and eta_phi must lie in (0, 1)");
  if (!(v.delta > 0.0) || !std::isfinite(v.delta)) return fail(IEM_E_ARG, "iem_search_create: delta must be positive");
  if (!(v.s_theta > 1.0) || !std::isfinite(v.s_theta)) return fail(IEM_E_ARG, "iem_search_create: s_theta must be greater than 1");
  if (!(v.s_phi >= 1.0) || !std::isfinite(v.s_phi)) return fail(IEM_E_ARG, "iem_search_create: s_phi must be at least 1");
  if (!(v.alpha_floor >= 0.0) || !std::isfinite(v.alpha_floor)) return fail(IEM_E_ARG, "iem_search_create: alpha_floor must be finite and not negative");
  if (v.max_trials < 1) return fail(IEM_E_ARG, "iem_search_create: max_trials must be at least 1");
  if (v.filter_capacity < 1 || v.filter_capacity > 1024) return fail(IEM_E_ARG, "iem_search_create: filter_capacity must lie in [1, 1024]");
  *out = v;
  return IEM_OK;
}
}  // namespace

int iem_search_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = object_source(kSearchSource, true, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_search_destroy(iem_search *s) {
  if (!s) return IEM_OK;
  DevGuard dg_(s->b->m->device);
  for (void *p : {(void *)s->d_ctl, (void *)s->d_filter, (void *)s->d_red, (void *)s->d_tab})
    if (p) hipFree(p);
  delete s;
  return IEM_OK;
}

int iem_search_create(iem_barrier *b, const iem_search_opts_t *opts, iem_search **out) {
  if (!b || !out) return fail(IEM_E_ARG, "null argument");
  iem_search_opts_t opt;
  {
    int rc = search_opts(opts, &opt);
    if (rc) return rc;
  }
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  {
    int rc = search_object(m);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_search *p) const { iem_search_destroy(p); } };      // (a failed create frees what it had allocated)
  std::unique_ptr<iem_search, Drop> s(new iem_search);
  s->b = b;
  s->opt = opt;
  const int64_t n_red = b->n_wg + 1 + (b->n_wg + 31) / 32;      // (IEM_TICKET_WORDS of csrc/iem_device.h)
  HIP_TRY(hipMalloc((void **)&s->d_ctl, 16 * 8));
  HIP_TRY(hipMalloc((void **)&s->d_filter, (size_t)opt.filter_capacity * 16));
  HIP_TRY(hipMalloc((void **)&s->d_red, (size_t)n_red * 8));
  HIP_TRY(hipMalloc((void **)&s->d_tab, 3 * 8));
  const long long tab[3] = {0, 0, (long long)b->n_wg};
  int64_t ctl[16] = {};
  ctl[9] = IEM_SEARCH_UNUSABLE;      // no begin yet: trial stores nothing, accept writes alpha = +0.0
  HIP_TRY(hipMemcpy(s->d_ctl, ctl, sizeof ctl, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(s->d_filter, 0, (size_t)opt.filter_capacity * 16));
  HIP_TRY(hipMemset(s->d_red, 0, (size_t)n_red * 8));
  HIP_TRY(hipMemcpy(s->d_tab, tab, sizeof tab, hipMemcpyHostToDevice));
  *out = s.release();
  return IEM_OK;
}

int iem_search_reset(iem_search *s) {
  if (!s) return fail(IEM_E_ARG, "null argument");
  iem_model *m = s->b->m;
  DevGuard dg_(m->device);
  HIP_TRY(hipMemsetAsync(s->d_ctl + 11, 0, 2 * 8, m->stream));      // the filter count and the flags
  return IEM_OK;
}

int iem_search_begin(iem_search *s, const double *d_x, const double *d_s, const double *d_grad, const double *d_sol, const double *d_ds, const double *d_obj,
                     const double *d_err, const double *d_alpha, double mu, double obj_weight) {
  if (!(s && s->mu_blk) && !(mu >= 0.0)) return fail(IEM_E_ARG, "iem_search_begin: mu must not be negative");
  if (!s || (s->b->nvar && (!d_x || !d_grad)) || (s->b->n_ineq && (!d_s || !d_ds)) || !d_sol || !d_obj || !d_err || !d_alpha) return fail(IEM_E_ARG, "null argument");
  iem_model *m = s->b->m;
  DevGuard dg_(m->device);
  SearchArgsH A = search_args(s);
  A.x = d_x; A.s = d_s; A.g = d_grad; A.sol = d_sol; A.ds = d_ds; A.obj = d_obj; A.err = d_err; A.alpha_in = d_alpha; A.mu = mu; A.sigma = obj_weight;
  return kkt_launch_raw(m, m->search.begin, &A, sizeof A, s->b->n_wg, 256);
}

int iem_search_trial(iem_search *s, const double *d_x, const double *d_s, const double *d_sol, const double *d_ds, double *d_xt, double *d_st) {
  if (!s || (s->b->nvar && (!d_x || !d_xt)) || (s->b->n_ineq && (!d_s || !d_ds || !d_st)) || !d_sol) return fail(IEM_E_ARG, "null argument");
  iem_model *m = s->b->m;
  DevGuard dg_(m->device);
  SearchArgsH A = search_args(s);
  A.x = d_x; A.s = d_s; A.sol = d_sol; A.ds = d_ds; A.xt = d_xt; A.st = d_st;
  return kkt_launch_raw(m, m->search.trial, &A, sizeof A, s->b->n_wg, 256);
}

int iem_search_accept(iem_search *s, const double *d_ft, const double *d_merit, double mu, double obj_weight, double *d_alpha) {
  if (!(s && s->mu_blk) && !(mu >= 0.0)) return fail(IEM_E_ARG, "iem_search_accept: mu must not be negative");
  if (!s || !d_ft || !d_merit || !d_alpha) return fail(IEM_E_ARG, "null argument");
  iem_model *m = s->b->m;
  DevGuard dg_(m->device);
  SearchArgsH A = search_args(s);
  A.ft = d_ft; A.merit = d_merit; A.alpha_out = d_alpha; A.mu = mu; A.sigma = obj_weight;
  return kkt_launch_raw(m, m->search.accept, &A, sizeof A, 1, 64);
}

int iem_search_device(const iem_search *s, void **d_control, double **d_filter) {
  if (!s) return fail(IEM_E_ARG, "null argument");
  if (d_control) *d_control = s->d_ctl;
  if (d_filter) *d_filter = s->d_filter;
  return IEM_OK;
}

int iem_search_state(iem_search *s, iem_search_state_t *out) {
  if (!s || !out) return fail(IEM_E_ARG, "null argument");
  if (out->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_search_state: set struct_size to sizeof(iem_search_state_t) before the call");
  iem_model *m = s->b->m;
  DevGuard dg_(m->device);
  uint64_t w[16];
  HIP_TRY(hipMemcpyAsync(w, s->d_ctl, sizeof w, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  iem_search_state_t v;
  static_assert(sizeof v == 14 * 8, "iem_search_state_t: struct_size, then words 0-12 of the block");
  v.struct_size = std::min<uint64_t>(out->struct_size, sizeof v);
  std::memcpy(&v.alpha, w, 13 * 8);
  std::memcpy(out, &v, (size_t)v.struct_size);      // never more than the caller's struct holds
  return IEM_OK;
}

/* ---- the second-order correction of the search: gate, corrected right-hand side, trial point, acceptance, selection (csrc/iem_soc_device.h) ---- */
struct iem_soc {
  iem_search *s = nullptr;
  iem_soc_opts_t opt;
  double *d_csoc = nullptr;            // the accumulated constraint residual: ncon
  const double *mu_blk = nullptr;      // iem_soc_bind_mu: the block of an iem_mu object (borrowed), or null
};

namespace {
// SocArgs of csrc/iem_soc_device.h
struct SocArgsH {
  const double *rl, *ru, *ceq;
  const unsigned char *fc;
  const double *x, *s, *y, *vL, *vU;
  const double *c, *ct, *st_in, *rhs;
  double *rhs_soc, *csoc;
  const double *sol, *ds, *dzL, *dzU, *dvL, *dvU;
  const double *alpha_soc;
  double *xt, *st;
  const double *ft, *merit;
  double *alpha_out;
  double *o_sol, *o_ds, *o_dzL, *o_dzU, *o_dvL, *o_dvU;
  double *ctl, *filter;
  double mu, sigma;
  double gamma_theta, gamma_phi, eta_phi, delta, s_theta, s_phi, kappa_soc;
  long long max_soc, capacity;
  long long nvar, n;
  const double *mu_blk;
};
SocArgsH soc_args(const iem_soc *q) {
  const iem_search *s = q->s;
  const iem_barrier *b = s->b;
  SocArgsH A;
  std::memset(&A, 0, sizeof A);
  A.rl = b->d_bounds + 2 * b->nvar; A.ru = A.rl + b->ncon; A.ceq = A.ru + b->ncon;
  A.fc = b->d_flags + b->nvar;
  A.csoc = q->d_csoc; A.ctl = s->d_ctl; A.filter = s->d_filter;
  A.gamma_theta = s->opt.gamma_theta; A.gamma_phi = s->opt.gamma_phi; A.eta_phi = s->opt.eta_phi; A.delta = s->opt.delta;
  A.s_theta = s->opt.s_theta; A.s_phi = s->opt.s_phi; A.kappa_soc = q->opt.kappa_soc;
  A.max_soc = (long long)q->opt.max_soc; A.capacity = (long long)s->opt.filter_capacity;
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon);
  A.mu_blk = q->mu_blk;
  return A;
}
const struct SocSlot { const char *name; hipFunction_t iem_model::SocObject::*fn; } kSocSlots[] = {
    {"soc_open", &iem_model::SocObject::open},     {"soc_rhs", &iem_model::SocObject::rhs},       {"soc_trial", &iem_model::SocObject::trial},
    {"soc_accept", &iem_model::SocObject::accept}, {"soc_select", &iem_model::SocObject::select},
};
int soc_object(iem_model *m) {
  iem_model::SocObject &o = m->soc;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = object_source(kSocSource, false, src);
  if (rc) return rc;
  KernelSlot slots[sizeof kSocSlots / sizeof *kSocSlots];
  int n = 0;
  for (const SocSlot &ss : kSocSlots) slots[n++] = KernelSlot{ss.name, &(o.*ss.fn)};
  return load_object(m, src, slots, n, &o.mod);
}
int soc_opts(const iem_soc_opts_t *in, iem_soc_opts_t *out) {
  iem_soc_opts_t v = {sizeof v, 4, 0.99};      // Ipopt's max_soc, kappa_soc
  if (in) {
    if (in->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_soc_create: set struct_size to sizeof(iem_soc_opts_t) before the call");
    std::memcpy(&v, in, (size_t)std::min<uint64_t>(in->struct_size, sizeof v));      // (fields a shorter struct does not have keep their defaults)
    v.struct_size = sizeof v;
  }
  if (v.max_soc < 1 || v.max_soc > 16) return fail(IEM_E_ARG, "iem_soc_create: max_soc must lie in [1, 16]");
  if (!(v.kappa_soc > 0.0) || !(v.kappa_soc <= 1.0)) return fail(IEM_E_ARG, "iem_soc_create: kappa_soc must lie in (0, 1]");
  *out = v;
  return IEM_OK;
}
}  // namespace

int iem_soc_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = object_source(kSocSource, false, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_soc_destroy(iem_soc *q) {
  if (!q) return IEM_OK;
  DevGuard dg_(q->s->b->m->device);
  if (q->d_csoc) hipFree(q->d_csoc);
  delete q;
  return IEM_OK;
}

int iem_soc_create(iem_search *s, const iem_soc_opts_t *opts, iem_soc **out) {
  if (!s || !out) return fail(IEM_E_ARG, "null argument");
  iem_soc_opts_t opt;
  {
    int rc = soc_opts(opts, &opt);
    if (rc) return rc;
  }
  iem_model *m = s->b->m;
  DevGuard dg_(m->device);
  {
    int rc = soc_object(m);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_soc *p) const { iem_soc_destroy(p); } };      // (a failed create frees what it had allocated)
  std::unique_ptr<iem_soc, Drop> q(new iem_soc);
  q->s = s;
  q->opt = opt;
  const size_t bytes = (size_t)std::max<int64_t>(s->b->ncon, 1) * 8;
  HIP_TRY(hipMalloc((void **)&q->d_csoc, bytes));
  HIP_TRY(hipMemset(q->d_csoc, 0, bytes));
  *out = q.release();
  return IEM_OK;
}

int iem_soc_open(iem_soc *q) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  iem_model *m = q->s->b->m;
  DevGuard dg_(m->device);
  SocArgsH A = soc_args(q);
  return kkt_launch_raw(m, m->soc.open, &A, sizeof A, 1, 64);
}

int iem_soc_rhs(iem_soc *q, const double *d_s, const double *d_y, const double *d_vL, const double *d_vU, const double *d_c, const double *d_ct, const double *d_st,
                const double *d_rhs, double mu, double *d_rhs_soc) {
  if (!(q && q->mu_blk) && !(mu >= 0.0)) return fail(IEM_E_ARG, "iem_soc_rhs: mu must not be negative");
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if ((b->ncon && (!d_c || !d_ct)) || (b->n_ineq && (!d_s || !d_y || !d_vL || !d_vU || !d_st)) || !d_rhs || !d_rhs_soc) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  SocArgsH A = soc_args(q);
  A.s = d_s; A.y = d_y; A.vL = d_vL; A.vU = d_vU; A.c = d_c; A.ct = d_ct; A.st_in = d_st; A.rhs = d_rhs; A.rhs_soc = d_rhs_soc; A.mu = mu;
  return kkt_launch_raw(m, m->soc.rhs, &A, sizeof A, b->n_wg, 256);
}

int iem_soc_trial(iem_soc *q, const double *d_x, const double *d_s, const double *d_sol_soc, const double *d_ds_soc, const double *d_alpha_soc, double *d_xt, double *d_st) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if ((b->nvar && (!d_x || !d_xt)) || (b->n_ineq && (!d_s || !d_ds_soc || !d_st)) || !d_sol_soc || !d_alpha_soc) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  SocArgsH A = soc_args(q);
  A.x = d_x; A.s = d_s; A.sol = d_sol_soc; A.ds = d_ds_soc; A.alpha_soc = d_alpha_soc; A.xt = d_xt; A.st = d_st;
  return kkt_launch_raw(m, m->soc.trial, &A, sizeof A, b->n_wg, 256);
}

int iem_soc_accept(iem_soc *q, const double *d_ft, const double *d_merit, const double *d_alpha_soc, double mu, double obj_weight, double *d_alpha) {
  if (!(q && q->mu_blk) && !(mu >= 0.0)) return fail(IEM_E_ARG, "iem_soc_accept: mu must not be negative");
  if (!q || !d_ft || !d_merit || !d_alpha_soc || !d_alpha) return fail(IEM_E_ARG, "null argument");
  iem_model *m = q->s->b->m;
  DevGuard dg_(m->device);
  SocArgsH A = soc_args(q);
  A.ft = d_ft; A.merit = d_merit; A.alpha_soc = d_alpha_soc; A.alpha_out = d_alpha; A.mu = mu; A.sigma = obj_weight;
  return kkt_launch_raw(m, m->soc.accept, &A, sizeof A, 1, 64);
}

int iem_soc_select(iem_soc *q, const double *d_sol_soc, const double *d_ds_soc, const double *d_dzL_soc, const double *d_dzU_soc, const double *d_dvL_soc,
                   const double *d_dvU_soc, double *d_sol, double *d_ds, double *d_dzL, double *d_dzU, double *d_dvL, double *d_dvU) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if (!d_sol_soc || !d_sol || (b->nvar && (!d_dzL_soc || !d_dzU_soc || !d_dzL || !d_dzU)) ||
      (b->n_ineq && (!d_ds_soc || !d_dvL_soc || !d_dvU_soc || !d_ds || !d_dvL || !d_dvU)))
    return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  SocArgsH A = soc_args(q);
  A.sol = d_sol_soc; A.ds = d_ds_soc; A.dzL = d_dzL_soc; A.dzU = d_dzU_soc; A.dvL = d_dvL_soc; A.dvU = d_dvU_soc;
  A.o_sol = d_sol; A.o_ds = d_ds; A.o_dzL = d_dzL; A.o_dzU = d_dzU; A.o_dvL = d_dvL; A.o_dvU = d_dvU;
  return kkt_launch_raw(m, m->soc.select, &A, sizeof A, b->n_wg, 256);
}

int iem_soc_device(const iem_soc *q, double **d_csoc) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  if (d_csoc) *d_csoc = q->d_csoc;
  return IEM_OK;
}

int iem_soc_state(iem_soc *q, iem_soc_state_t *out) {
  if (!q || !out) return fail(IEM_E_ARG, "null argument");
  if (out->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_soc_state: set struct_size to sizeof(iem_soc_state_t) before the call");
  iem_model *m = q->s->b->m;
  DevGuard dg_(m->device);
  uint64_t w[16];
  HIP_TRY(hipMemcpyAsync(w, q->s->d_ctl, sizeof w, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  iem_soc_state_t v;
  static_assert(sizeof v == 5 * 8, "iem_soc_state_t: struct_size, the status word, then words 13-15 of the block");
  v.struct_size = std::min<uint64_t>(out->struct_size, sizeof v);
  std::memcpy(&v.status, w + 9, 8);
  std::memcpy(&v.state, w + 13, 3 * 8);
  std::memcpy(out, &v, (size_t)v.struct_size);      // never more than the caller's struct holds
  return IEM_OK;
}

/* ---- the feasibility restoration phase: elastic start, terms, step, merit, inner search, return test (csrc/iem_resto_device.h) ---- */
struct iem_resto {
  iem_search *s = nullptr;             // the ORIGINAL problem's search (borrowed): its filter and control block
  iem_search *inner = nullptr;         // the restoration problem's own search (owned), on the same barrier object
  iem_resto_opts_t opt;
  double *d_vec = nullptr;             // p | n | zp | zn | dp | dn | dzp | dzn | pt | nt | sR | ws (ncon each) | xR | wx (nvar each)
  double *d_blk = nullptr;             // the block: 8 words
  double *d_red = nullptr;             // 4 n_wg parked values + the ticket words (zeroed once; the tickets reset themselves)
  const double *mu_blk = nullptr;      // iem_resto_bind_mu: the restoration block of an iem_rmu object (borrowed), or null
  const double *mu_orig_blk = nullptr; // ... and the ORIGINAL problem's iem_mu block that object was given, or null
};

namespace {
// RestoArgs of csrc/iem_resto_device.h
struct RestoArgsH {
  const double *xl, *xu, *rl, *ru, *ceq;
  const unsigned char *fx, *fc;
  double *x, *s, *y, *zL, *zU, *vL, *vU;
  const double *r, *c, *sol;
  double *ds, *dzL, *dzU, *dvL, *dvU;
  double *sigma, *dcon, *rhs;
  unsigned long long *alpha;
  double *out;
  double *xt, *st;
  const double *merit0, *f, *merit;
  double *p, *n_, *zp, *zn, *dp, *dn, *dzp, *dzn, *pt, *nt, *sR, *ws, *xR, *wx;
  double *blk;
  double *octl, *ofilter;
  double *ictl;
  double *red;
  const long long *tab;
  double mu, tau, kappa, zeta, rho, kappa_resto, threshold, gamma_theta, gamma_phi;
  long long capacity, which;
  long long nvar, n, n_wg;
  const double *mu_blk, *mu_orig_blk;
};
enum { RES_ENTER, RES_ENTER_FILTER, RES_TERMS, RES_STEP, RES_MERIT, RES_BEGIN, RES_TRIAL, RES_UPDATE, RES_ERROR, RES_CHECK, RES_LEAVE_MAX, RES_LEAVE, RES_KERNELS };
const char *const kRestoKernels[RES_KERNELS] = {"resto_enter", "resto_enter_filter", "resto_terms", "resto_step", "resto_merit", "resto_begin",
                                                "resto_trial", "resto_update", "resto_error", "resto_check", "resto_leave_max", "resto_leave"};
RestoArgsH resto_args(const iem_resto *q) {
  const iem_search *s = q->s;
  const iem_barrier *b = s->b;
  RestoArgsH A;
  std::memset(&A, 0, sizeof A);
  A.xl = b->d_bounds; A.xu = A.xl + b->nvar; A.rl = A.xu + b->nvar; A.ru = A.rl + b->ncon; A.ceq = A.ru + b->ncon;
  A.fx = b->d_flags; A.fc = A.fx + b->nvar;
  double *v = q->d_vec;
  const int64_t m = b->ncon;
  A.p = v; A.n_ = v + m; A.zp = v + 2 * m; A.zn = v + 3 * m; A.dp = v + 4 * m; A.dn = v + 5 * m; A.dzp = v + 6 * m; A.dzn = v + 7 * m;
  A.pt = v + 8 * m; A.nt = v + 9 * m; A.sR = v + 10 * m; A.ws = v + 11 * m; A.xR = v + 12 * m; A.wx = A.xR + b->nvar;
  A.blk = q->d_blk; A.octl = s->d_ctl; A.ofilter = s->d_filter; A.ictl = q->inner->d_ctl;
  A.red = q->d_red; A.tab = b->d_tab;
  A.rho = q->opt.rho; A.kappa_resto = q->opt.kappa_resto; A.threshold = q->opt.bound_mult_reset_threshold;
  A.gamma_theta = s->opt.gamma_theta; A.gamma_phi = s->opt.gamma_phi; A.capacity = (long long)s->opt.filter_capacity;
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon); A.n_wg = (long long)b->n_wg;
  A.mu_blk = q->mu_blk; A.mu_orig_blk = q->mu_orig_blk;
  return A;
}
int resto_object(iem_model *m) {
  iem_model::RestoObject &o = m->resto;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = object_source(kRestoSource, true, src);
  if (rc) return rc;
  KernelSlot slots[RES_KERNELS];
  for (int k = 0; k < RES_KERNELS; ++k) slots[k] = KernelSlot{kRestoKernels[k], &o.fn[k]};
  return load_object(m, src, slots, RES_KERNELS, &o.mod);
}
// unbound: the restoration object as it always was (its RestoArgs ends in front of mu_blk); bound: the variant below, which reads the block
int resto_launch(const iem_resto *q, int which, RestoArgsH &A, bool one_wave = false) {
  iem_model *m = q->s->b->m;
  const long long grid = one_wave ? 1 : q->s->b->n_wg;
  if (A.mu_blk) return kkt_launch_raw(m, m->resto_mu.fn[which], &A, sizeof A, grid, one_wave ? 64 : 256);
  return kkt_launch_raw(m, m->resto.fn[which], &A, offsetof(RestoArgsH, mu_blk), grid, one_wave ? 64 : 256);
}
// The BOUND variant of the restoration code object: the text of csrc/iem_resto_device.h with RestoArgs two pointers longer and the
// single read of mu, tau and zeta in every kernel that takes one taken from the restoration block {mu, tau, zeta, ...}; resto_check
// takes the ORIGINAL problem's mu from word 0 of the original block where there is one — derived from the one text, so that the
// unbound object keeps its source, its key and its bits, and the two cannot drift apart.  Every pattern must match exactly as often
// as listed: an edit of the header that breaks one is an error here, not a silently unbound kernel.
int resto_mu_source(std::string &s) {
  static const struct { const char *from, *to; int times; } kEdits[] = {
      {"  long long nvar, n, n_wg;\n};",
       "  long long nvar, n, n_wg;\n  const double *mu_blk, *mu_orig_blk;      // the restoration block {mu, tau, zeta, ...}; the ORIGINAL iem_mu block or null\n};", 1},
      {"  const double mu = A.mu, rho = A.rho, rho2 = 2.0 * A.rho;\n", "  const double mu = A.mu_blk[0], rho = A.rho, rho2 = 2.0 * A.rho;\n", 1},      // resto_enter
      {"  const double mu = A.mu, zeta = A.zeta;\n", "  const double mu = A.mu_blk[0], zeta = A.mu_blk[2];\n", 1},      // resto_terms
      {"  const double mu = A.mu, tau = A.tau, ntau = -A.tau, zeta = A.zeta;\n",
       "  const double mu = A.mu_blk[0], tau = A.mu_blk[1], ntau = -tau, zeta = A.mu_blk[2];\n", 1},      // resto_step
      {"(0.5 * A.zeta) * lds[1]", "(0.5 * A.mu_blk[2]) * lds[1]", 1},      // resto_merit
      {"  const double mu = A.mu, zeta = A.zeta, rho = A.rho;\n", "  const double mu = A.mu_blk[0], zeta = A.mu_blk[2], rho = A.rho;\n", 2},      // resto_begin, resto_error
      {"  const double mu = A.mu, kappa = A.kappa;\n", "  const double mu = A.mu_blk[0], kappa = A.kappa;\n", 1},      // resto_update
      {"A.f[0] - A.mu * A.merit[1]", "A.f[0] - (A.mu_orig_blk ? A.mu_orig_blk[0] : A.mu) * A.merit[1]", 1},      // resto_check
  };
  std::string text(kRestoSource);
  for (const auto &e : kEdits) {
    const std::string from(e.from), to(e.to);
    int seen = 0;
    for (size_t at = text.find(from); at != std::string::npos; at = text.find(from, at + to.size())) {
      text.replace(at, from.size(), to);
      ++seen;
    }
    if (seen != e.times) return fail(IEM_E_COMPILE, std::string("internal: the restoration kernels do not read mu where the bound variant expects it: ") + e.from);
  }
  if (text.find("A.mu,") != std::string::npos || text.find("A.tau") != std::string::npos || text.find("A.zeta") != std::string::npos)
    return fail(IEM_E_COMPILE, "internal: the bound variant of the restoration kernels still reads a host scalar");
  return object_source(text.c_str(), true, s);
}
int resto_mu_object(iem_model *m) {
  iem_model::RestoObject &o = m->resto_mu;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = resto_mu_source(src);
  if (rc) return rc;
  KernelSlot slots[RES_KERNELS];
  for (int k = 0; k < RES_KERNELS; ++k) slots[k] = KernelSlot{kRestoKernels[k], &o.fn[k]};
  return load_object(m, src, slots, RES_KERNELS, &o.mod);
}
int resto_opts(const iem_resto_opts_t *in, iem_resto_opts_t *out) {
  iem_resto_opts_t v = {sizeof v, 1000.0, 0.9, 1000.0};      // Ipopt's rho, required_infeasibility_reduction, bound_mult_reset_threshold
  if (in) {
    if (in->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_resto_create: set struct_size to sizeof(iem_resto_opts_t) before the call");
    std::memcpy(&v, in, (size_t)std::min<uint64_t>(in->struct_size, sizeof v));      // (fields a shorter struct does not have keep their defaults)
    v.struct_size = sizeof v;
  }
  if (!(v.rho > 0.0) || !std::isfinite(v.rho)) return fail(IEM_E_ARG, "iem_resto_create: rho must be positive");
  if (!(v.kappa_resto > 0.0) || !(v.kappa_resto < 1.0)) return fail(IEM_E_ARG, "iem_resto_create: kappa_resto must lie in (0, 1)");
  if (!(v.bound_mult_reset_threshold >= 0.0)) return fail(IEM_E_ARG, "iem_resto_create: bound_mult_reset_threshold must not be negative");
  *out = v;
  return IEM_OK;
}
// mu, zeta, tau as every call checks them
int resto_scalars(const char *call, double mu, double zeta, double tau = 1.0) {
  if (!(mu >= 0.0)) return fail(IEM_E_ARG, std::string(call) + ": mu must not be negative");
  if (!(zeta >= 0.0)) return fail(IEM_E_ARG, std::string(call) + ": zeta must not be negative");
  if (!(tau > 0.0 && tau <= 1.0)) return fail(IEM_E_ARG, std::string(call) + ": tau must lie in (0, 1]");
  return IEM_OK;
}
void resto_set_state(RestoArgsH &A, const double *x, const double *s, const double *y, const double *zL, const double *zU, const double *vL, const double *vU) {
  A.x = (double *)x; A.s = (double *)s; A.y = (double *)y; A.zL = (double *)zL; A.zU = (double *)zU; A.vL = (double *)vL; A.vU = (double *)vU;
}
}  // namespace

int iem_resto_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = object_source(kRestoSource, true, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_resto_destroy(iem_resto *q) {
  if (!q) return IEM_OK;
  DevGuard dg_(q->s->b->m->device);
  if (q->inner) iem_search_destroy(q->inner);
  for (void *p : {(void *)q->d_vec, (void *)q->d_blk, (void *)q->d_red})
    if (p) hipFree(p);
  delete q;
  return IEM_OK;
}

int iem_resto_create(iem_search *fs, const iem_resto_opts_t *opts, iem_resto **out) {
  if (!fs || !out) return fail(IEM_E_ARG, "null argument");
  iem_resto_opts_t opt;
  {
    int rc = resto_opts(opts, &opt);
    if (rc) return rc;
  }
  iem_barrier *b = fs->b;
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  {
    int rc = resto_object(m);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_resto *p) const { iem_resto_destroy(p); } };      // (a failed create frees what it had allocated)
  std::unique_ptr<iem_resto, Drop> q(new iem_resto);
  q->s = fs;
  q->opt = opt;
  {
    int rc = iem_search_create(b, &fs->opt, &q->inner);      // the restoration problem's own filter, with the options of the original search
    if (rc) return rc;
  }
  const size_t n_vec = (size_t)std::max<int64_t>(12 * b->ncon + 2 * b->nvar, 1);
  const int64_t n_red = 4 * b->n_wg + 1 + (b->n_wg + 31) / 32;      // (IEM_TICKET_WORDS of csrc/iem_device.h)
  HIP_TRY(hipMalloc((void **)&q->d_vec, n_vec * 8));
  HIP_TRY(hipMalloc((void **)&q->d_blk, 8 * 8));
  HIP_TRY(hipMalloc((void **)&q->d_red, (size_t)n_red * 8));
  HIP_TRY(hipMemset(q->d_vec, 0, n_vec * 8));
  HIP_TRY(hipMemset(q->d_blk, 0, 8 * 8));
  HIP_TRY(hipMemset(q->d_red, 0, (size_t)n_red * 8));
  *out = q.release();
  return IEM_OK;
}

int iem_resto_search(const iem_resto *q, iem_search **out_inner) {
  if (!q || !out_inner) return fail(IEM_E_ARG, "null argument");
  *out_inner = q->inner;
  return IEM_OK;
}

int iem_resto_enter(iem_resto *q, const double *d_x, const double *d_s, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU, const double *d_c,
                    double mu) {
  int rc = q && q->mu_blk ? IEM_OK : resto_scalars("iem_resto_enter", mu, 0.0);      // (bound: the block rules, the host scalars are ignored)
  if (rc) return rc;
  if (!q || barrier_state_missing(q->s->b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || (q->s->b->ncon && !d_c)) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(q->s->b->m->device);
  RestoArgsH A = resto_args(q);
  resto_set_state(A, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU);
  A.c = d_c; A.mu = mu;
  if ((rc = resto_launch(q, RES_ENTER, A))) return rc;
  return resto_launch(q, RES_ENTER_FILTER, A, true);
}

int iem_resto_terms(iem_resto *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                    const double *d_vU, const double *d_r, const double *d_c, double mu, double zeta, double *d_sigma, double *d_dcon, double *d_rhs) {
  int rc = q && q->mu_blk ? IEM_OK : resto_scalars("iem_resto_terms", mu, zeta);      // (bound: the block rules, the host scalars are ignored)
  if (rc) return rc;
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if (barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || (b->nvar && (!d_r || !d_sigma)) || (b->ncon && (!d_c || !d_dcon)) || !d_rhs)
    return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(b->m->device);
  RestoArgsH A = resto_args(q);
  resto_set_state(A, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU);
  A.r = d_r; A.c = d_c; A.mu = mu; A.zeta = zeta; A.sigma = d_sigma; A.dcon = d_dcon; A.rhs = d_rhs;
  return resto_launch(q, RES_TERMS, A);
}

int iem_resto_step(iem_resto *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                   const double *d_vU, const double *d_sol, double mu, double tau, double zeta, double *d_ds, double *d_dzL, double *d_dzU,
                   double *d_dvL, double *d_dvU, double *d_alpha) {
  int rc = q && q->mu_blk ? IEM_OK : resto_scalars("iem_resto_step", mu, zeta, tau);      // (bound: the block rules, the host scalars are ignored)
  if (rc) return rc;
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if (barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || !d_sol || !d_alpha || (b->nvar && (!d_dzL || !d_dzU)) ||
      (b->n_ineq && (!d_ds || !d_dvL || !d_dvU)))
    return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  RestoArgsH A = resto_args(q);
  resto_set_state(A, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU);
  A.sol = d_sol; A.mu = mu; A.tau = tau; A.zeta = zeta; A.ds = d_ds; A.dzL = d_dzL; A.dzU = d_dzU; A.dvL = d_dvL; A.dvU = d_dvU;
  A.alpha = (unsigned long long *)d_alpha;
  HIP_TRY(hipMemcpyAsync(d_alpha, b->d_ones, 16, hipMemcpyDeviceToDevice, m->stream));      // the seed: the bits of 1.0
  return resto_launch(q, RES_STEP, A);
}

int iem_resto_merit(iem_resto *q, int which, const double *d_x, const double *d_s, const double *d_c, double zeta, double *d_out) {
  int rc = q && q->mu_blk ? IEM_OK : resto_scalars("iem_resto_merit", 0.0, zeta);      // (bound: the block rules, the host scalars are ignored)
  if (rc) return rc;
  if (which != 0 && which != 1) return fail(IEM_E_ARG, "iem_resto_merit: which must be 0 (the state) or 1 (the trial point)");
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if ((b->nvar && !d_x) || (b->n_ineq && !d_s) || (b->ncon && !d_c) || !d_out) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(b->m->device);
  RestoArgsH A = resto_args(q);
  A.x = (double *)d_x; A.s = (double *)d_s; A.c = d_c; A.zeta = zeta; A.out = d_out; A.which = which;
  return resto_launch(q, RES_MERIT, A);
}

int iem_resto_begin(iem_resto *q, const double *d_x, const double *d_s, const double *d_sol, const double *d_ds, const double *d_merit0, const double *d_alpha,
                    double mu, double zeta) {
  int rc = q && q->mu_blk ? IEM_OK : resto_scalars("iem_resto_begin", mu, zeta);      // (bound: the block rules, the host scalars are ignored)
  if (rc) return rc;
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if ((b->nvar && !d_x) || (b->n_ineq && (!d_s || !d_ds)) || !d_sol || !d_merit0 || !d_alpha) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(b->m->device);
  RestoArgsH A = resto_args(q);
  A.x = (double *)d_x; A.s = (double *)d_s; A.sol = d_sol; A.ds = (double *)d_ds; A.merit0 = d_merit0; A.alpha = (unsigned long long *)d_alpha; A.mu = mu; A.zeta = zeta;
  return resto_launch(q, RES_BEGIN, A);
}

int iem_resto_trial(iem_resto *q, const double *d_x, const double *d_s, const double *d_sol, const double *d_ds, double *d_xt, double *d_st) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if ((b->nvar && (!d_x || !d_xt)) || (b->n_ineq && (!d_s || !d_ds || !d_st)) || !d_sol) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(b->m->device);
  RestoArgsH A = resto_args(q);
  A.x = (double *)d_x; A.s = (double *)d_s; A.sol = d_sol; A.ds = (double *)d_ds; A.xt = d_xt; A.st = d_st;
  return resto_launch(q, RES_TRIAL, A);
}

int iem_resto_update(iem_resto *q, double *d_x, double *d_s, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU, const double *d_sol,
                     const double *d_ds, const double *d_dzL, const double *d_dzU, const double *d_dvL, const double *d_dvU, const double *d_alpha, double mu,
                     double kappa_sigma) {
  int rc = q && q->mu_blk ? IEM_OK : resto_scalars("iem_resto_update", mu, 0.0);      // (bound: the block rules, the host scalars are ignored)
  if (rc) return rc;
  if (!(kappa_sigma >= 1.0)) return fail(IEM_E_ARG, "iem_resto_update: kappa_sigma must be at least 1");
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if (barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || !d_sol || !d_alpha || (b->nvar && (!d_dzL || !d_dzU)) ||
      (b->n_ineq && (!d_ds || !d_dvL || !d_dvU)))
    return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(b->m->device);
  RestoArgsH A = resto_args(q);
  resto_set_state(A, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU);
  A.sol = d_sol; A.ds = (double *)d_ds; A.dzL = (double *)d_dzL; A.dzU = (double *)d_dzU; A.dvL = (double *)d_dvL; A.dvU = (double *)d_dvU;
  A.alpha = (unsigned long long *)d_alpha; A.mu = mu; A.kappa = kappa_sigma;
  return resto_launch(q, RES_UPDATE, A);
}

int iem_resto_error(iem_resto *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                    const double *d_vU, const double *d_r, const double *d_c, double mu, double zeta, double *d_out) {
  int rc = q && q->mu_blk ? IEM_OK : resto_scalars("iem_resto_error", mu, zeta);      // (bound: the block rules, the host scalars are ignored)
  if (rc) return rc;
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if (barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || (b->ncon && !d_c) || !d_out) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  RestoArgsH A = resto_args(q);
  resto_set_state(A, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU);
  A.r = d_r; A.c = d_c; A.mu = mu; A.zeta = zeta; A.out = d_out;
  HIP_TRY(hipMemsetAsync(d_out, 0, 4 * 8, m->stream));      // the four maxima start from +0.0
  return resto_launch(q, RES_ERROR, A);
}

int iem_resto_check(iem_resto *q, const double *d_f, const double *d_merit, double mu) {
  int rc = q && q->mu_orig_blk ? IEM_OK : resto_scalars("iem_resto_check", mu, 0.0);      // (bound with an original block: that block rules)
  if (rc) return rc;
  if (!q || !d_f || !d_merit) return fail(IEM_E_ARG, "null argument");
  DevGuard dg_(q->s->b->m->device);
  RestoArgsH A = resto_args(q);
  A.f = d_f; A.merit = d_merit; A.mu = mu;
  return resto_launch(q, RES_CHECK, A, true);
}

int iem_resto_leave(iem_resto *q, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->s->b;
  if ((b->nvar && (!d_zL || !d_zU)) || (b->ncon && !d_y) || (b->n_ineq && (!d_vL || !d_vU))) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  RestoArgsH A = resto_args(q);
  A.y = d_y; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU;
  HIP_TRY(hipMemsetAsync(q->d_blk + 4, 0, 8, m->stream));      // the maximum starts from +0.0
  int rc = resto_launch(q, RES_LEAVE_MAX, A);
  return rc ? rc : resto_launch(q, RES_LEAVE, A);
}

int iem_resto_device(const iem_resto *q, double **d_p, double **d_n, double **d_zp, double **d_zn, void **d_block) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const int64_t m = q->s->b->ncon;
  if (d_p) *d_p = q->d_vec;
  if (d_n) *d_n = q->d_vec + m;
  if (d_zp) *d_zp = q->d_vec + 2 * m;
  if (d_zn) *d_zn = q->d_vec + 3 * m;
  if (d_block) *d_block = q->d_blk;
  return IEM_OK;
}

int iem_resto_state(iem_resto *q, iem_resto_state_t *out) {
  if (!q || !out) return fail(IEM_E_ARG, "null argument");
  if (out->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_resto_state: set struct_size to sizeof(iem_resto_state_t) before the call");
  iem_model *m = q->s->b->m;
  DevGuard dg_(m->device);
  uint64_t w[8];
  HIP_TRY(hipMemcpyAsync(w, q->d_blk, sizeof w, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  iem_resto_state_t v;
  static_assert(sizeof v == 5 * 8, "iem_resto_state_t: struct_size, then words 0-3 of the block");
  v.struct_size = std::min<uint64_t>(out->struct_size, sizeof v);
  std::memcpy(&v.state, w, 4 * 8);
  std::memcpy(out, &v, (size_t)v.struct_size);      // never more than the caller's struct holds
  return IEM_OK;
}

/* ---- the barrier parameter on the device: error terms, the monotone rule, the block the other objects read (csrc/iem_mu_device.h) ---- */
struct iem_mu {
  iem_barrier *b = nullptr;
  iem_mu_opts_t opt;                   // mu_floor resolved
  double *d_blk = nullptr;             // the block: 16 words
  double *d_red = nullptr;             // 6 n_wg parked values + the ticket words (zeroed once; the tickets reset themselves)
  long long *d_tab = nullptr;          // offs[6] | first[6] | count[6] of iem_shared_totals
  double *d_seed = nullptr;            // what the twelve words of iem_mu_error start from: +0.0, and the bits of +inf in word 8
};

namespace {
// MuArgs of csrc/iem_mu_device.h
struct MuArgsH {
  const double *xl, *xu, *rl, *ru, *ceq;
  const unsigned char *fx, *fc;
  const double *x, *s, *y, *zL, *zU, *vL, *vU;
  const double *r, *c;
  double *out;
  const double *w;
  double *blk;
  double *sctl;
  double *red;
  const long long *tab;
  double kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max, mu0;
  long long ncon, nz;
  long long nvar, n, n_wg;
};
MuArgsH mu_args(const iem_mu *p) {
  const iem_barrier *b = p->b;
  MuArgsH A;
  std::memset(&A, 0, sizeof A);
  A.xl = b->d_bounds; A.xu = A.xl + b->nvar; A.rl = A.xu + b->nvar; A.ru = A.rl + b->ncon; A.ceq = A.ru + b->ncon;
  A.fx = b->d_flags; A.fc = A.fx + b->nvar;
  A.blk = p->d_blk; A.red = p->d_red; A.tab = p->d_tab;
  A.kappa_eps = p->opt.kappa_eps; A.kappa_mu = p->opt.kappa_mu; A.tau_min = p->opt.tau_min; A.tol = p->opt.tol; A.mu_floor = p->opt.mu_floor; A.s_max = p->opt.s_max;
  A.ncon = (long long)b->ncon; A.nz = (long long)(b->n_xl + b->n_xu + b->n_sl + b->n_su);
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon); A.n_wg = (long long)b->n_wg;
  return A;
}
int mu_object(iem_model *m) {
  iem_model::MuObject &o = m->mu;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = object_source(kMuSource, true, src);
  if (rc) return rc;
  KernelSlot slots[3] = {KernelSlot{"mu_error", &o.error}, KernelSlot{"mu_update", &o.update}, KernelSlot{"mu_reset", &o.reset}};
  return load_object(m, src, slots, 3, &o.mod);
}
int mu_opts(const iem_mu_opts_t *in, iem_mu_opts_t *out) {
  iem_mu_opts_t v = {sizeof v, 0.1, 10.0, 0.2, 0.99, 1e-8, 0.0, 100.0};      // Ipopt's mu_init, barrier_tol_factor, mu_linear_decrease_factor, tau_min, tol; s_max
  if (in) {
    if (in->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_mu_create: set struct_size to sizeof(iem_mu_opts_t) before the call");
    std::memcpy(&v, in, (size_t)std::min<uint64_t>(in->struct_size, sizeof v));      // (fields a shorter struct does not have keep their defaults)
    v.struct_size = sizeof v;
  }
  for (double f : {v.mu_init, v.kappa_eps, v.kappa_mu, v.tau_min, v.tol, v.mu_floor, v.s_max})
    if (!std::isfinite(f)) return fail(IEM_E_ARG, "iem_mu_create: every option must be finite");
  auto unit = [](double g) { return g > 0.0 && g < 1.0; };
  if (!(v.mu_init > 0.0)) return fail(IEM_E_ARG, "iem_mu_create: mu_init must be positive");
  if (!unit(v.kappa_mu) || !unit(v.tau_min)) return fail(IEM_E_ARG, "iem_mu_create: kappa_mu and tau_min must lie in (0, 1)");
  if (!(v.kappa_eps > 0.0)) return fail(IEM_E_ARG, "iem_mu_create: kappa_eps must be positive");
  if (!(v.tol > 0.0)) return fail(IEM_E_ARG, "iem_mu_create: tol must be positive");
  if (!(v.mu_floor >= 0.0)) return fail(IEM_E_ARG, "iem_mu_create: mu_floor must not be negative");
  if (!(v.s_max > 0.0)) return fail(IEM_E_ARG, "iem_mu_create: s_max must be positive");
  if (v.mu_floor == 0.0) v.mu_floor = std::max(1e-11, v.tol / 10.0);
  *out = v;
  return IEM_OK;
}
}  // namespace

int iem_barrier_mu_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = barrier_mu_source(s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_mu_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = object_source(kMuSource, true, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_mu_destroy(iem_mu *p) {
  if (!p) return IEM_OK;
  DevGuard dg_(p->b->m->device);
  for (void *q : {(void *)p->d_blk, (void *)p->d_red, (void *)p->d_tab, (void *)p->d_seed})
    if (q) hipFree(q);
  delete p;
  return IEM_OK;
}

int iem_mu_create(iem_barrier *b, const iem_mu_opts_t *opts, iem_mu **out) {
  if (!b || !out) return fail(IEM_E_ARG, "null argument");
  iem_mu_opts_t opt;
  {
    int rc = mu_opts(opts, &opt);
    if (rc) return rc;
  }
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  {
    int rc = mu_object(m);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_mu *p) const { iem_mu_destroy(p); } };      // (a failed create frees what it had allocated)
  std::unique_ptr<iem_mu, Drop> p(new iem_mu);
  p->b = b;
  p->opt = opt;
  const int64_t n_red = 6 * b->n_wg + 1 + (b->n_wg + 31) / 32;      // (IEM_TICKET_WORDS of csrc/iem_device.h)
  HIP_TRY(hipMalloc((void **)&p->d_blk, 16 * 8));
  HIP_TRY(hipMalloc((void **)&p->d_red, (size_t)n_red * 8));
  HIP_TRY(hipMalloc((void **)&p->d_tab, 18 * 8));
  HIP_TRY(hipMalloc((void **)&p->d_seed, 12 * 8));
  long long tab[18];
  for (int s = 0; s < 6; ++s) { tab[s] = s * (long long)b->n_wg; tab[6 + s] = 0; tab[12 + s] = (long long)b->n_wg; }
  double seed[12] = {};
  seed[8] = std::numeric_limits<double>::infinity();
  double blk[16] = {};      // status ITERATING, no flag, counters 0
  blk[0] = opt.mu_init;
  blk[1] = std::max(opt.tau_min, 1.0 - opt.mu_init);
  blk[2] = std::sqrt(opt.mu_init);
  HIP_TRY(hipMemcpy(p->d_blk, blk, sizeof blk, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(p->d_red, 0, (size_t)n_red * 8));
  HIP_TRY(hipMemcpy(p->d_tab, tab, sizeof tab, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->d_seed, seed, sizeof seed, hipMemcpyHostToDevice));
  *out = p.release();
  return IEM_OK;
}

int iem_mu_reset(iem_mu *p, double mu0) {
  if (!p) return fail(IEM_E_ARG, "null argument");
  if (!(mu0 > 0.0) || !std::isfinite(mu0)) return fail(IEM_E_ARG, "iem_mu_reset: mu0 must be positive and finite");
  iem_model *m = p->b->m;
  DevGuard dg_(m->device);
  MuArgsH A = mu_args(p);
  A.mu0 = mu0;
  return kkt_launch_raw(m, m->mu.reset, &A, sizeof A, 1, 64);
}

int iem_mu_error(iem_mu *p, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
                 const double *d_r, const double *d_c, double *d_out) {
  if (!p || barrier_state_missing(p->b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || (p->b->nvar && !d_r) || (p->b->ncon && !d_c) || !d_out)
    return fail(IEM_E_ARG, "null argument");
  iem_model *m = p->b->m;
  DevGuard dg_(m->device);
  MuArgsH A = mu_args(p);
  A.x = d_x; A.s = d_s; A.y = d_y; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU; A.r = d_r; A.c = d_c; A.out = d_out;
  // the seed: the maxima start from +0.0, the minimum from the bits of +inf (a device-to-device copy is a capturable node)
  HIP_TRY(hipMemcpyAsync(d_out, p->d_seed, 12 * 8, hipMemcpyDeviceToDevice, m->stream));
  return kkt_launch_raw(m, m->mu.error, &A, sizeof A, p->b->n_wg, 256);
}

int iem_mu_update(iem_mu *p, const double *d_out12, iem_search *fs) {
  if (!p || !d_out12) return fail(IEM_E_ARG, "null argument");
  if (fs && fs->b != p->b) return fail(IEM_E_ARG, "iem_mu_update: the search belongs to another barrier object");
  iem_model *m = p->b->m;
  DevGuard dg_(m->device);
  MuArgsH A = mu_args(p);
  A.w = d_out12;
  A.sctl = fs ? fs->d_ctl : nullptr;
  return kkt_launch_raw(m, m->mu.update, &A, sizeof A, 1, 64);
}

int iem_mu_device(const iem_mu *p, double **d_block) {
  if (!p) return fail(IEM_E_ARG, "null argument");
  if (d_block) *d_block = p->d_blk;
  return IEM_OK;
}

int iem_mu_state(iem_mu *p, iem_mu_state_t *out) {
  if (!p || !out) return fail(IEM_E_ARG, "null argument");
  if (out->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_mu_state: set struct_size to sizeof(iem_mu_state_t) before the call");
  iem_model *m = p->b->m;
  DevGuard dg_(m->device);
  uint64_t w[16];
  HIP_TRY(hipMemcpyAsync(w, p->d_blk, sizeof w, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  iem_mu_state_t v;
  static_assert(sizeof v == 13 * 8, "iem_mu_state_t: struct_size, then words 0-11 of the block");
  v.struct_size = std::min<uint64_t>(out->struct_size, sizeof v);
  std::memcpy(&v.mu, w, 12 * 8);
  std::memcpy(out, &v, (size_t)v.struct_size);      // never more than the caller's struct holds
  return IEM_OK;
}

int iem_barrier_bind_mu(iem_barrier *b, const iem_mu *p) {
  if (!b) return fail(IEM_E_ARG, "null argument");
  if (p && p->b != b) return fail(IEM_E_ARG, "iem_barrier_bind_mu: the iem_mu object was created on another barrier object");
  if (p) {
    DevGuard dg_(b->m->device);
    int rc = barrier_mu_object(b->m);
    if (rc) return rc;
  }
  b->mu_blk = p ? p->d_blk : nullptr;
  return IEM_OK;
}

int iem_search_bind_mu(iem_search *fs, const iem_mu *p) {
  if (!fs) return fail(IEM_E_ARG, "null argument");
  if (p && p->b != fs->b) return fail(IEM_E_ARG, "iem_search_bind_mu: the iem_mu object was created on another barrier object");
  fs->mu_blk = p ? p->d_blk : nullptr;
  return IEM_OK;
}

int iem_soc_bind_mu(iem_soc *q, const iem_mu *p) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  if (p && p->b != q->s->b) return fail(IEM_E_ARG, "iem_soc_bind_mu: the iem_mu object was created on another barrier object");
  q->mu_blk = p ? p->d_blk : nullptr;
  return IEM_OK;
}

/* ---- the adaptive barrier parameter: the probing oracle's look along the affine direction, the free / fixed rule on an iem_mu block (csrc/iem_amu_device.h) ---- */
struct iem_amu {
  iem_mu *p = nullptr;                 // the object whose block it drives (borrowed)
  iem_amu_opts_t opt;
  double *d_blk = nullptr;             // the own block: 16 words
  double *d_red = nullptr;             // 2 n_wg parked values + the ticket words (zeroed once; the tickets reset themselves)
  long long *d_tab = nullptr;          // offs[2] | first[2] | count[2] of iem_shared_totals
};

namespace {
// AmuArgs of csrc/iem_amu_device.h
struct AmuArgsH {
  const double *xl, *xu, *rl, *ru;
  const unsigned char *fx, *fc;
  const double *x, *s, *zL, *zU, *vL, *vU;
  const double *sol, *ds, *dzL, *dzU, *dvL, *dvU;
  const double *alpha;
  double *out;
  const double *w;
  const double *probe;
  double *mblk;
  double *ablk;
  double *sctl;
  double *red;
  const long long *tab;
  double kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max;
  double sigma_max, mu_min, mu_max_fact, init_factor, red_fact;
  long long refs_max, oracle, force_fixed;
  long long ncon, nz;
  long long nvar, n, n_wg;
};
AmuArgsH amu_args(const iem_amu *a) {
  const iem_mu *p = a->p;
  const iem_barrier *b = p->b;
  AmuArgsH A;
  std::memset(&A, 0, sizeof A);
  A.xl = b->d_bounds; A.xu = A.xl + b->nvar; A.rl = A.xu + b->nvar; A.ru = A.rl + b->ncon;
  A.fx = b->d_flags; A.fc = A.fx + b->nvar;
  A.mblk = p->d_blk; A.ablk = a->d_blk; A.red = a->d_red; A.tab = a->d_tab;
  A.kappa_eps = p->opt.kappa_eps; A.kappa_mu = p->opt.kappa_mu; A.tau_min = p->opt.tau_min; A.tol = p->opt.tol; A.mu_floor = p->opt.mu_floor; A.s_max = p->opt.s_max;
  A.sigma_max = a->opt.sigma_max; A.mu_min = a->opt.mu_min; A.mu_max_fact = a->opt.mu_max_fact; A.init_factor = a->opt.init_factor; A.red_fact = a->opt.red_fact;
  A.refs_max = (long long)a->opt.refs_max; A.oracle = (long long)a->opt.oracle;
  A.ncon = (long long)b->ncon; A.nz = (long long)(b->n_xl + b->n_xu + b->n_sl + b->n_su);
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon); A.n_wg = (long long)b->n_wg;
  return A;
}
int amu_object(iem_model *m) {
  iem_model::AmuObject &o = m->amu;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = object_source(kAmuSource, true, src);
  if (rc) return rc;
  KernelSlot slots[3] = {KernelSlot{"amu_probe", &o.probe}, KernelSlot{"amu_update", &o.update}, KernelSlot{"amu_reset", &o.reset}};
  return load_object(m, src, slots, 3, &o.mod);
}
int amu_opts(const iem_amu_opts_t *in, iem_amu_opts_t *out) {
  iem_amu_opts_t v = {sizeof v, IEM_AMU_PROBING, 100.0, 1e-11, 1e3, 0.8, 0.9999, 4};      // Ipopt's sigma_max, mu_min, adaptive_mu_kkterror_red_fact / _red_iters, adaptive_mu_monotone_init_factor; mu_max_fact
  if (in) {
    if (in->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_amu_create: set struct_size to sizeof(iem_amu_opts_t) before the call");
    std::memcpy(&v, in, (size_t)std::min<uint64_t>(in->struct_size, sizeof v));      // (fields a shorter struct does not have keep their defaults)
    v.struct_size = sizeof v;
  }
  for (double f : {v.sigma_max, v.mu_min, v.mu_max_fact, v.init_factor, v.red_fact})
    if (!std::isfinite(f)) return fail(IEM_E_ARG, "iem_amu_create: every option must be finite");
  if (v.oracle != IEM_AMU_PROBING && v.oracle != IEM_AMU_LOQO) return fail(IEM_E_ARG, "iem_amu_create: oracle must be 0 (probing) or 1 (LOQO)");
  if (!(v.sigma_max > 0.0)) return fail(IEM_E_ARG, "iem_amu_create: sigma_max must be positive");
  if (!(v.mu_min > 0.0)) return fail(IEM_E_ARG, "iem_amu_create: mu_min must be positive");
  if (!(v.mu_max_fact > 0.0)) return fail(IEM_E_ARG, "iem_amu_create: mu_max_fact must be positive");
  if (!(v.init_factor > 0.0)) return fail(IEM_E_ARG, "iem_amu_create: init_factor must be positive");
  if (!(v.red_fact > 0.0 && v.red_fact < 1.0)) return fail(IEM_E_ARG, "iem_amu_create: red_fact must lie in (0, 1)");
  if (v.refs_max < 1 || v.refs_max > 4) return fail(IEM_E_ARG, "iem_amu_create: refs_max must lie in 1..4");
  *out = v;
  return IEM_OK;
}
}  // namespace

int iem_amu_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = object_source(kAmuSource, true, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_amu_destroy(iem_amu *a) {
  if (!a) return IEM_OK;
  DevGuard dg_(a->p->b->m->device);
  for (void *q : {(void *)a->d_blk, (void *)a->d_red, (void *)a->d_tab})
    if (q) hipFree(q);
  delete a;
  return IEM_OK;
}

int iem_amu_create(iem_mu *p, const iem_amu_opts_t *opts, iem_amu **out) {
  if (!p || !out) return fail(IEM_E_ARG, "null argument");
  iem_amu_opts_t opt;
  {
    int rc = amu_opts(opts, &opt);
    if (rc) return rc;
  }
  const iem_barrier *b = p->b;
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  {
    int rc = amu_object(m);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_amu *a) const { iem_amu_destroy(a); } };      // (a failed create frees what it had allocated)
  std::unique_ptr<iem_amu, Drop> a(new iem_amu);
  a->p = p;
  a->opt = opt;
  const int64_t n_red = 2 * b->n_wg + 1 + (b->n_wg + 31) / 32;      // (IEM_TICKET_WORDS of csrc/iem_device.h)
  HIP_TRY(hipMalloc((void **)&a->d_blk, 16 * 8));
  HIP_TRY(hipMalloc((void **)&a->d_red, (size_t)n_red * 8));
  HIP_TRY(hipMalloc((void **)&a->d_tab, 6 * 8));
  long long tab[6];
  for (int s = 0; s < 2; ++s) { tab[s] = s * (long long)b->n_wg; tab[2 + s] = 0; tab[4 + s] = (long long)b->n_wg; }
  int64_t blk[16] = {};      // mode FREE, mu_max unset, the ring empty, counters 0
  blk[13] = opt.oracle;
  HIP_TRY(hipMemcpy(a->d_blk, blk, sizeof blk, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(a->d_red, 0, (size_t)n_red * 8));
  HIP_TRY(hipMemcpy(a->d_tab, tab, sizeof tab, hipMemcpyHostToDevice));
  *out = a.release();
  return IEM_OK;
}

int iem_amu_reset(iem_amu *a) {
  if (!a) return fail(IEM_E_ARG, "null argument");
  iem_model *m = a->p->b->m;
  DevGuard dg_(m->device);
  AmuArgsH A = amu_args(a);
  return kkt_launch_raw(m, m->amu.reset, &A, sizeof A, 1, 64);
}

int iem_amu_probe(iem_amu *a, const double *d_x, const double *d_s, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
                  const double *d_sol, const double *d_ds, const double *d_dzL, const double *d_dzU, const double *d_dvL, const double *d_dvU,
                  const double *d_alpha, double *d_out) {
  if (!a || !d_sol || !d_alpha || !d_out) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = a->p->b;
  if ((b->nvar && (!d_x || !d_zL || !d_zU || !d_dzL || !d_dzU)) || (b->n_ineq && (!d_s || !d_vL || !d_vU || !d_ds || !d_dvL || !d_dvU))) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  AmuArgsH A = amu_args(a);
  A.x = d_x; A.s = d_s; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU;
  A.sol = d_sol; A.ds = d_ds; A.dzL = d_dzL; A.dzU = d_dzU; A.dvL = d_dvL; A.dvU = d_dvU;
  A.alpha = d_alpha; A.out = d_out;
  return kkt_launch_raw(m, m->amu.probe, &A, sizeof A, b->n_wg, 256);      // no seed: the last arrival writes all four words
}

int iem_amu_update(iem_amu *a, const double *d_out12, const double *d_probe4, int force_fixed, iem_search *fs) {
  if (!a || !d_out12) return fail(IEM_E_ARG, "null argument");
  if (a->opt.oracle == IEM_AMU_PROBING && !d_probe4) return fail(IEM_E_ARG, "iem_amu_update: the probing oracle needs the four words of iem_amu_probe");
  if (fs && fs->b != a->p->b) return fail(IEM_E_ARG, "iem_amu_update: the search belongs to another barrier object");
  iem_model *m = a->p->b->m;
  DevGuard dg_(m->device);
  AmuArgsH A = amu_args(a);
  A.w = d_out12;
  A.probe = a->opt.oracle == IEM_AMU_PROBING ? d_probe4 : nullptr;
  A.force_fixed = force_fixed ? 1 : 0;
  A.sctl = fs ? fs->d_ctl : nullptr;
  return kkt_launch_raw(m, m->amu.update, &A, sizeof A, 1, 64);
}

int iem_amu_device(const iem_amu *a, double **d_block) {
  if (!a) return fail(IEM_E_ARG, "null argument");
  if (d_block) *d_block = a->d_blk;
  return IEM_OK;
}

int iem_amu_state(iem_amu *a, iem_mu_state_t *mu_out, iem_amu_state_t *out) {
  if (!a || !mu_out || !out) return fail(IEM_E_ARG, "null argument");
  if (mu_out->struct_size < sizeof(uint64_t) || out->struct_size < sizeof(uint64_t))
    return fail(IEM_E_ARG, "iem_amu_state: set struct_size to sizeof(iem_mu_state_t) / sizeof(iem_amu_state_t) before the call");
  iem_model *m = a->p->b->m;
  DevGuard dg_(m->device);
  uint64_t w[32];
  HIP_TRY(hipMemcpyAsync(w, a->p->d_blk, 16 * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipMemcpyAsync(w + 16, a->d_blk, 16 * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));      // ONE synchronisation for both blocks
  iem_mu_state_t v;
  v.struct_size = std::min<uint64_t>(mu_out->struct_size, sizeof v);
  std::memcpy(&v.mu, w, 12 * 8);
  std::memcpy(mu_out, &v, (size_t)v.struct_size);      // never more than the caller's struct holds
  iem_amu_state_t u;
  static_assert(sizeof u == 15 * 8, "iem_amu_state_t: struct_size, then words 0-13 of the own block");
  u.struct_size = std::min<uint64_t>(out->struct_size, sizeof u);
  std::memcpy(&u.mode, w + 16, 14 * 8);
  std::memcpy(out, &u, (size_t)u.struct_size);
  return IEM_OK;
}

/* ---- the quality-function oracle: residual norms, step lengths and the quality function at a candidate sigma, the section search, the rule (csrc/iem_qf_device.h) ---- */
struct iem_qf {
  iem_amu *a = nullptr;                // the object whose rule it completes (borrowed), on its iem_mu
  iem_qf_opts_t opt;                   // sigma_max resolved: the iem_amu object's where the caller gave 0
  double *d_blk = nullptr;             // the own block: 32 words
  double *d_red = nullptr;             // 2 n_wg parked values + the ticket words (zeroed once; the tickets reset themselves)
  long long *d_tab = nullptr;          // offs[2] | first[2] | count[2] of iem_shared_totals
};

namespace {
// QfArgs of csrc/iem_qf_device.h
struct QfArgsH {
  const double *xl, *xu, *rl, *ru, *ceq;
  const unsigned char *fx, *fc;
  const double *x, *s, *y, *zL, *zU, *vL, *vU;
  const double *r, *c;
  const double *sol0, *ds0, *dzL0, *dzU0, *dvL0, *dvU0;
  const double *sol1, *ds1, *dzL1, *dzU1, *dvL1, *dvU1;
  const double *w;
  double *mblk;
  double *ablk;
  double *qblk;
  double *sctl;
  double *red;
  const long long *tab;
  double kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max;
  double mu_min, mu_max_fact, init_factor, red_fact;
  double mu_ref, sigma_min, sigma_max, sigma_tol;
  long long max_steps, refs_max, force_fixed;
  long long n_d, n_p;
  long long ncon, nz;
  long long nvar, n, n_wg;
};
QfArgsH qf_args(const iem_qf *q) {
  const iem_amu *a = q->a;
  const iem_mu *p = a->p;
  const iem_barrier *b = p->b;
  QfArgsH A;
  std::memset(&A, 0, sizeof A);
  A.xl = b->d_bounds; A.xu = A.xl + b->nvar; A.rl = A.xu + b->nvar; A.ru = A.rl + b->ncon; A.ceq = A.ru + b->ncon;
  A.fx = b->d_flags; A.fc = A.fx + b->nvar;
  A.mblk = p->d_blk; A.ablk = a->d_blk; A.qblk = q->d_blk; A.red = q->d_red; A.tab = q->d_tab;
  A.kappa_eps = p->opt.kappa_eps; A.kappa_mu = p->opt.kappa_mu; A.tau_min = p->opt.tau_min; A.tol = p->opt.tol; A.mu_floor = p->opt.mu_floor; A.s_max = p->opt.s_max;
  A.mu_min = a->opt.mu_min; A.mu_max_fact = a->opt.mu_max_fact; A.init_factor = a->opt.init_factor; A.red_fact = a->opt.red_fact;
  A.mu_ref = q->opt.mu_ref; A.sigma_min = q->opt.sigma_min; A.sigma_max = q->opt.sigma_max; A.sigma_tol = q->opt.section_sigma_tol;
  A.max_steps = (long long)q->opt.max_section_steps; A.refs_max = (long long)a->opt.refs_max;
  A.n_d = (long long)(b->nvar + b->n_ineq); A.n_p = (long long)b->ncon;
  A.ncon = (long long)b->ncon; A.nz = (long long)(b->n_xl + b->n_xu + b->n_sl + b->n_su);
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon); A.n_wg = (long long)b->n_wg;
  return A;
}
int qf_object(iem_model *m) {
  iem_model::QfObject &o = m->qf;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = object_source(kQfSource, true, src);
  if (rc) return rc;
  KernelSlot slots[5] = {KernelSlot{"qf_begin", &o.begin}, KernelSlot{"qf_alpha", &o.alpha}, KernelSlot{"qf_value", &o.value}, KernelSlot{"qf_update", &o.update},
                         KernelSlot{"qf_reset", &o.reset}};
  return load_object(m, src, slots, 5, &o.mod);
}
int qf_opts(const iem_qf_opts_t *in, double amu_sigma_max, iem_qf_opts_t *out) {
  iem_qf_opts_t v = {sizeof v, 1.0, 1e-6, 0.0, 1e-2, 8};      // mu_ref; Ipopt's sigma_min; sigma_max (0: the iem_amu object's); quality_function_section_sigma_tol, quality_function_max_section_steps
  if (in) {
    if (in->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_qf_create: set struct_size to sizeof(iem_qf_opts_t) before the call");
    std::memcpy(&v, in, (size_t)std::min<uint64_t>(in->struct_size, sizeof v));      // (fields a shorter struct does not have keep their defaults)
    v.struct_size = sizeof v;
  }
  for (double f : {v.mu_ref, v.sigma_min, v.sigma_max, v.section_sigma_tol})
    if (!std::isfinite(f)) return fail(IEM_E_ARG, "iem_qf_create: every option must be finite");
  if (!(v.mu_ref > 0.0)) return fail(IEM_E_ARG, "iem_qf_create: mu_ref must be positive");
  if (!(v.sigma_min > 0.0)) return fail(IEM_E_ARG, "iem_qf_create: sigma_min must be positive");
  if (v.sigma_max < 0.0) return fail(IEM_E_ARG, "iem_qf_create: sigma_max must be positive (or 0: the iem_amu object's)");
  if (!(v.section_sigma_tol > 0.0)) return fail(IEM_E_ARG, "iem_qf_create: section_sigma_tol must be positive");
  if (v.max_section_steps < 1 || v.max_section_steps > 16) return fail(IEM_E_ARG, "iem_qf_create: max_section_steps must lie in 1..16");
  if (v.sigma_max == 0.0) v.sigma_max = amu_sigma_max;
  *out = v;
  return IEM_OK;
}
}  // namespace

int iem_qf_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = object_source(kQfSource, true, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_qf_destroy(iem_qf *q) {
  if (!q) return IEM_OK;
  DevGuard dg_(q->a->p->b->m->device);
  for (void *v : {(void *)q->d_blk, (void *)q->d_red, (void *)q->d_tab})
    if (v) hipFree(v);
  delete q;
  return IEM_OK;
}

int iem_qf_create(iem_amu *a, const iem_qf_opts_t *opts, iem_qf **out) {
  if (!a || !out) return fail(IEM_E_ARG, "null argument");
  iem_qf_opts_t opt;
  {
    int rc = qf_opts(opts, a->opt.sigma_max, &opt);
    if (rc) return rc;
  }
  const iem_barrier *b = a->p->b;
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  {
    int rc = qf_object(m);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_qf *q) const { iem_qf_destroy(q); } };      // (a failed create frees what it had allocated)
  std::unique_ptr<iem_qf, Drop> q(new iem_qf);
  q->a = a;
  q->opt = opt;
  const int64_t n_red = 2 * b->n_wg + 1 + (b->n_wg + 31) / 32;      // (IEM_TICKET_WORDS of csrc/iem_device.h)
  HIP_TRY(hipMalloc((void **)&q->d_blk, 32 * 8));
  HIP_TRY(hipMalloc((void **)&q->d_red, (size_t)n_red * 8));
  HIP_TRY(hipMalloc((void **)&q->d_tab, 6 * 8));
  long long tab[6];
  for (int s = 0; s < 2; ++s) { tab[s] = s * (long long)b->n_wg; tab[2 + s] = 0; tab[4 + s] = (long long)b->n_wg; }
  HIP_TRY(hipMemset(q->d_blk, 0, 32 * 8));      // status IDLE: alpha and value do nothing before the first begin
  HIP_TRY(hipMemset(q->d_red, 0, (size_t)n_red * 8));
  HIP_TRY(hipMemcpy(q->d_tab, tab, sizeof tab, hipMemcpyHostToDevice));
  *out = q.release();
  return IEM_OK;
}

int iem_qf_reset(iem_qf *q) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  iem_model *m = q->a->p->b->m;
  DevGuard dg_(m->device);
  QfArgsH A = qf_args(q);
  return kkt_launch_raw(m, m->qf.reset, &A, sizeof A, 1, 64);
}

int iem_qf_begin(iem_qf *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
                 const double *d_r, const double *d_c, const double *d_out12) {
  if (!q || !d_out12) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->a->p->b;
  if ((b->nvar && (!d_x || !d_zL || !d_zU || !d_r)) || (b->ncon && (!d_y || !d_c)) || (b->n_ineq && (!d_s || !d_vL || !d_vU))) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  QfArgsH A = qf_args(q);
  A.x = d_x; A.s = d_s; A.y = d_y; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU;
  A.r = d_r; A.c = d_c; A.w = d_out12;
  return kkt_launch_raw(m, m->qf.begin, &A, sizeof A, b->n_wg, 256);      // no seed: the last arrival writes the whole block
}

namespace {
// the arguments iem_qf_alpha and iem_qf_value share
int qf_pair(iem_qf *q, bool value, const double *d_x, const double *d_s, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
            const double *const *d0, const double *const *d1) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->a->p->b;
  if ((b->nvar && (!d_x || !d_zL || !d_zU || !d0[0] || !d1[0] || !d0[2] || !d0[3] || !d1[2] || !d1[3])) ||
      (b->n_ineq && (!d_s || !d_vL || !d_vU || !d0[1] || !d1[1] || !d0[4] || !d0[5] || !d1[4] || !d1[5])))
    return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  QfArgsH A = qf_args(q);
  A.x = d_x; A.s = d_s; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU;
  A.sol0 = d0[0]; A.ds0 = d0[1]; A.dzL0 = d0[2]; A.dzU0 = d0[3]; A.dvL0 = d0[4]; A.dvU0 = d0[5];
  A.sol1 = d1[0]; A.ds1 = d1[1]; A.dzL1 = d1[2]; A.dzU1 = d1[3]; A.dvL1 = d1[4]; A.dvU1 = d1[5];
  return kkt_launch_raw(m, value ? m->qf.value : m->qf.alpha, &A, sizeof A, b->n_wg, 256);
}
}  // namespace

int iem_qf_alpha(iem_qf *q, const double *d_x, const double *d_s, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
                 const double *d_sol0, const double *d_ds0, const double *d_dzL0, const double *d_dzU0, const double *d_dvL0, const double *d_dvU0,
                 const double *d_sol1, const double *d_ds1, const double *d_dzL1, const double *d_dzU1, const double *d_dvL1, const double *d_dvU1) {
  const double *d0[6] = {d_sol0, d_ds0, d_dzL0, d_dzU0, d_dvL0, d_dvU0}, *d1[6] = {d_sol1, d_ds1, d_dzL1, d_dzU1, d_dvL1, d_dvU1};
  return qf_pair(q, false, d_x, d_s, d_zL, d_zU, d_vL, d_vU, d0, d1);
}

int iem_qf_value(iem_qf *q, const double *d_x, const double *d_s, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
                 const double *d_sol0, const double *d_ds0, const double *d_dzL0, const double *d_dzU0, const double *d_dvL0, const double *d_dvU0,
                 const double *d_sol1, const double *d_ds1, const double *d_dzL1, const double *d_dzU1, const double *d_dvL1, const double *d_dvU1) {
  const double *d0[6] = {d_sol0, d_ds0, d_dzL0, d_dzU0, d_dvL0, d_dvU0}, *d1[6] = {d_sol1, d_ds1, d_dzL1, d_dzU1, d_dvL1, d_dvU1};
  return qf_pair(q, true, d_x, d_s, d_zL, d_zU, d_vL, d_vU, d0, d1);
}

int iem_qf_update(iem_qf *q, const double *d_out12, int force_fixed, iem_search *fs) {
  if (!q || !d_out12) return fail(IEM_E_ARG, "null argument");
  if (fs && fs->b != q->a->p->b) return fail(IEM_E_ARG, "iem_qf_update: the search belongs to another barrier object");
  iem_model *m = q->a->p->b->m;
  DevGuard dg_(m->device);
  QfArgsH A = qf_args(q);
  A.w = d_out12;
  A.force_fixed = force_fixed ? 1 : 0;
  A.sctl = fs ? fs->d_ctl : nullptr;
  return kkt_launch_raw(m, m->qf.update, &A, sizeof A, 1, 64);
}

int iem_qf_device(const iem_qf *q, double **d_block) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  if (d_block) *d_block = q->d_blk;
  return IEM_OK;
}

int iem_qf_state(iem_qf *q, iem_mu_state_t *mu_out, iem_amu_state_t *amu_out, iem_qf_state_t *out) {
  if (!q || !mu_out || !amu_out || !out) return fail(IEM_E_ARG, "null argument");
  if (mu_out->struct_size < sizeof(uint64_t) || amu_out->struct_size < sizeof(uint64_t) || out->struct_size < sizeof(uint64_t))
    return fail(IEM_E_ARG, "iem_qf_state: set struct_size to sizeof(iem_mu_state_t) / sizeof(iem_amu_state_t) / sizeof(iem_qf_state_t) before the call");
  iem_model *m = q->a->p->b->m;
  DevGuard dg_(m->device);
  uint64_t w[64];
  HIP_TRY(hipMemcpyAsync(w, q->a->p->d_blk, 16 * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipMemcpyAsync(w + 16, q->a->d_blk, 16 * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipMemcpyAsync(w + 32, q->d_blk, 32 * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));      // ONE synchronisation for the three blocks
  iem_mu_state_t v;
  v.struct_size = std::min<uint64_t>(mu_out->struct_size, sizeof v);
  std::memcpy(&v.mu, w, 12 * 8);
  std::memcpy(mu_out, &v, (size_t)v.struct_size);      // never more than the caller's struct holds
  iem_amu_state_t u;
  u.struct_size = std::min<uint64_t>(amu_out->struct_size, sizeof u);
  std::memcpy(&u.mode, w + 16, 14 * 8);
  std::memcpy(amu_out, &u, (size_t)u.struct_size);
  iem_qf_state_t t;
  static_assert(sizeof t == 28 * 8, "iem_qf_state_t: struct_size, then words 0-26 of the own block");
  t.struct_size = std::min<uint64_t>(out->struct_size, sizeof t);
  std::memcpy(&t.status, w + 32, 27 * 8);
  std::memcpy(out, &t, (size_t)t.struct_size);
  return IEM_OK;
}

/* ---- Mehrotra's corrector: the two-column right-hand side, the corrected directions and step lengths, the safeguard's decision (csrc/iem_mpc_device.h) ---- */
struct iem_mpc {
  iem_amu *a = nullptr;                // the object whose affine direction it completes (borrowed), on its iem_mu
  iem_mpc_opts_t opt;
  double *d_blk = nullptr;             // the own block: 16 words
  const double *mu_blk = nullptr;      // iem_mpc_bind_mu: the block of the iem_mu object (borrowed), or null
};

namespace {
// MpcArgs of csrc/iem_mpc_device.h
struct MpcArgsH {
  const double *xl, *xu, *rl, *ru, *ceq;
  const unsigned char *fx, *fc;
  const double *x, *s, *y, *zL, *zU, *vL, *vU;
  const double *r, *c;
  const double *sol_a, *ds_a, *dzL_a, *dzU_a, *dvL_a, *dvU_a;
  const double *sol;
  double *ds, *dzL, *dzU, *dvL, *dvU;
  double *rhs0, *rhs1;
  unsigned long long *alpha;
  const double *probe;
  double *o_sol, *o_ds, *o_dzL, *o_dzU, *o_dvL, *o_dvU, *o_alpha;
  const double *mblk;
  const double *ablk;
  double *blk;
  double mu, tau, red_fact;
  long long nz;
  long long nvar, n;
};
MpcArgsH mpc_args(const iem_mpc *q) {
  const iem_barrier *b = q->a->p->b;
  MpcArgsH A;
  std::memset(&A, 0, sizeof A);
  A.xl = b->d_bounds; A.xu = A.xl + b->nvar; A.rl = A.xu + b->nvar; A.ru = A.rl + b->ncon; A.ceq = A.ru + b->ncon;
  A.fx = b->d_flags; A.fc = A.fx + b->nvar;
  A.mblk = q->mu_blk; A.ablk = q->a->d_blk; A.blk = q->d_blk;
  A.red_fact = q->opt.red_fact;
  A.nz = (long long)(b->n_xl + b->n_xu + b->n_sl + b->n_su);
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon);
  return A;
}
int mpc_object(iem_model *m) {
  iem_model::MpcObject &o = m->mpc;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = object_source(kMpcSource, true, src);
  if (rc) return rc;
  KernelSlot slots[4] = {KernelSlot{"mpc_terms", &o.terms}, KernelSlot{"mpc_step", &o.step}, KernelSlot{"mpc_select", &o.select}, KernelSlot{"mpc_reset", &o.reset}};
  return load_object(m, src, slots, 4, &o.mod);
}
int mpc_opts(const iem_mpc_opts_t *in, iem_mpc_opts_t *out) {
  iem_mpc_opts_t v = {sizeof v, 1.0};      // Ipopt's corrector_compl_avrg_red_fact
  if (in) {
    if (in->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_mpc_create: set struct_size to sizeof(iem_mpc_opts_t) before the call");
    std::memcpy(&v, in, (size_t)std::min<uint64_t>(in->struct_size, sizeof v));      // (fields a shorter struct does not have keep their defaults)
    v.struct_size = sizeof v;
  }
  if (!std::isfinite(v.red_fact) || !(v.red_fact > 0.0)) return fail(IEM_E_ARG, "iem_mpc_create: red_fact must be positive and finite");
  *out = v;
  return IEM_OK;
}
// the affine direction a call needs: dx, dzL, dzU with variables, ds, dvL, dvU with inequality rows
bool mpc_affine_missing(const iem_barrier *b, const double *sol, const double *ds, const double *dzL, const double *dzU, const double *dvL, const double *dvU) {
  return !sol || (b->nvar && (!dzL || !dzU)) || (b->n_ineq && (!ds || !dvL || !dvU));
}
}  // namespace

int iem_mpc_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = object_source(kMpcSource, true, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_mpc_destroy(iem_mpc *q) {
  if (!q) return IEM_OK;
  DevGuard dg_(q->a->p->b->m->device);
  if (q->d_blk) hipFree(q->d_blk);
  delete q;
  return IEM_OK;
}

int iem_mpc_create(iem_amu *a, const iem_mpc_opts_t *opts, iem_mpc **out) {
  if (!a || !out) return fail(IEM_E_ARG, "null argument");
  iem_mpc_opts_t opt;
  {
    int rc = mpc_opts(opts, &opt);
    if (rc) return rc;
  }
  iem_model *m = a->p->b->m;
  DevGuard dg_(m->device);
  {
    int rc = mpc_object(m);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_mpc *q) const { iem_mpc_destroy(q); } };      // (a failed create frees what it had allocated)
  std::unique_ptr<iem_mpc, Drop> q(new iem_mpc);
  q->a = a;
  q->opt = opt;
  HIP_TRY(hipMalloc((void **)&q->d_blk, 16 * 8));
  HIP_TRY(hipMemset(q->d_blk, 0, 16 * 8));
  *out = q.release();
  return IEM_OK;
}

int iem_mpc_reset(iem_mpc *q) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  iem_model *m = q->a->p->b->m;
  DevGuard dg_(m->device);
  MpcArgsH A = mpc_args(q);
  return kkt_launch_raw(m, m->mpc.reset, &A, sizeof A, 1, 64);
}

int iem_mpc_bind_mu(iem_mpc *q, const iem_mu *p) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  if (p && p != q->a->p) return fail(IEM_E_ARG, "iem_mpc_bind_mu: not the iem_mu object this corrector was created on");
  q->mu_blk = p ? p->d_blk : nullptr;
  return IEM_OK;
}

int iem_mpc_terms(iem_mpc *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                  const double *d_vU, const double *d_r, const double *d_c, const double *d_sol_aff, const double *d_ds_aff, const double *d_dzL_aff,
                  const double *d_dzU_aff, const double *d_dvL_aff, const double *d_dvU_aff, double mu, double *d_rhs2, int64_t ld) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  if (!q->mu_blk && !(mu >= 0.0)) return fail(IEM_E_ARG, "iem_mpc_terms: mu must not be negative");
  const iem_barrier *b = q->a->p->b;
  if (barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || (b->nvar && !d_r) || (b->ncon && !d_c) || !d_rhs2 ||
      mpc_affine_missing(b, d_sol_aff, d_ds_aff, d_dzL_aff, d_dzU_aff, d_dvL_aff, d_dvU_aff))
    return fail(IEM_E_ARG, "null argument");
  if (ld < b->nvar + b->ncon) return fail(IEM_E_ARG, "iem_mpc_terms: ld must be at least nvar + ncon");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  MpcArgsH A = mpc_args(q);
  A.x = d_x; A.s = d_s; A.y = d_y; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU; A.r = d_r; A.c = d_c;
  A.sol_a = d_sol_aff; A.ds_a = d_ds_aff; A.dzL_a = d_dzL_aff; A.dzU_a = d_dzU_aff; A.dvL_a = d_dvL_aff; A.dvU_a = d_dvU_aff;
  A.mu = mu; A.rhs0 = d_rhs2; A.rhs1 = d_rhs2 + ld;
  return kkt_launch_raw(m, m->mpc.terms, &A, sizeof A, b->n_wg, 256);
}

int iem_mpc_step(iem_mpc *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                 const double *d_vU, const double *d_sol_aff, const double *d_ds_aff, const double *d_dzL_aff, const double *d_dzU_aff,
                 const double *d_dvL_aff, const double *d_dvU_aff, const double *d_sol_c, double mu, double tau, double *d_ds_c, double *d_dzL_c,
                 double *d_dzU_c, double *d_dvL_c, double *d_dvU_c, double *d_alpha_c) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  if (!q->mu_blk && !(mu >= 0.0)) return fail(IEM_E_ARG, "iem_mpc_step: mu must not be negative");
  if (!q->mu_blk && !(tau > 0.0 && tau <= 1.0)) return fail(IEM_E_ARG, "iem_mpc_step: tau must lie in (0, 1]");
  const iem_barrier *b = q->a->p->b;
  if (barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || !d_sol_c || !d_alpha_c ||
      mpc_affine_missing(b, d_sol_aff, d_ds_aff, d_dzL_aff, d_dzU_aff, d_dvL_aff, d_dvU_aff) ||
      mpc_affine_missing(b, d_sol_c, d_ds_c, d_dzL_c, d_dzU_c, d_dvL_c, d_dvU_c))
    return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  MpcArgsH A = mpc_args(q);
  A.x = d_x; A.s = d_s; A.y = d_y; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU;
  A.sol_a = d_sol_aff; A.ds_a = d_ds_aff; A.dzL_a = d_dzL_aff; A.dzU_a = d_dzU_aff; A.dvL_a = d_dvL_aff; A.dvU_a = d_dvU_aff;
  A.sol = d_sol_c; A.mu = mu; A.tau = tau; A.ds = d_ds_c; A.dzL = d_dzL_c; A.dzU = d_dzU_c; A.dvL = d_dvL_c; A.dvU = d_dvU_c;
  A.alpha = (unsigned long long *)d_alpha_c;
  // the seed: the bits of 1.0 (the barrier object's; a device-to-device copy is a capturable node)
  HIP_TRY(hipMemcpyAsync(d_alpha_c, b->d_ones, 16, hipMemcpyDeviceToDevice, m->stream));
  return kkt_launch_raw(m, m->mpc.step, &A, sizeof A, b->n_wg, 256);
}

int iem_mpc_select(iem_mpc *q, const double *d_probe4, const double *d_alpha_c, const double *d_sol_c, const double *d_ds_c, const double *d_dzL_c,
                   const double *d_dzU_c, const double *d_dvL_c, const double *d_dvU_c, double *d_sol, double *d_ds, double *d_dzL, double *d_dzU,
                   double *d_dvL, double *d_dvU, double *d_alpha) {
  if (!q || !d_probe4 || !d_alpha_c || !d_alpha) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->a->p->b;
  if (mpc_affine_missing(b, d_sol_c, d_ds_c, d_dzL_c, d_dzU_c, d_dvL_c, d_dvU_c) || mpc_affine_missing(b, d_sol, d_ds, d_dzL, d_dzU, d_dvL, d_dvU))
    return fail(IEM_E_ARG, "null argument");
  if (d_alpha == d_alpha_c) return fail(IEM_E_ARG, "iem_mpc_select: d_alpha and d_alpha_c must be two buffers (every thread reads the one while one thread writes the other)");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  MpcArgsH A = mpc_args(q);
  A.probe = d_probe4; A.alpha = (unsigned long long *)d_alpha_c;
  A.sol = d_sol_c; A.ds = (double *)d_ds_c; A.dzL = (double *)d_dzL_c; A.dzU = (double *)d_dzU_c; A.dvL = (double *)d_dvL_c; A.dvU = (double *)d_dvU_c;
  A.o_sol = d_sol; A.o_ds = d_ds; A.o_dzL = d_dzL; A.o_dzU = d_dzU; A.o_dvL = d_dvL; A.o_dvU = d_dvU; A.o_alpha = d_alpha;
  return kkt_launch_raw(m, m->mpc.select, &A, sizeof A, b->n_wg, 256);
}

int iem_mpc_device(const iem_mpc *q, double **d_block) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  if (d_block) *d_block = q->d_blk;
  return IEM_OK;
}

int iem_mpc_state(iem_mpc *q, iem_mpc_state_t *out) {
  if (!q || !out) return fail(IEM_E_ARG, "null argument");
  if (out->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_mpc_state: set struct_size to sizeof(iem_mpc_state_t) before the call");
  iem_model *m = q->a->p->b->m;
  DevGuard dg_(m->device);
  uint64_t w[16];
  HIP_TRY(hipMemcpyAsync(w, q->d_blk, sizeof w, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  iem_mpc_state_t v;
  static_assert(sizeof v == 8 * 8, "iem_mpc_state_t: struct_size, then words 0-6 of the own block");
  v.struct_size = std::min<uint64_t>(out->struct_size, sizeof v);
  std::memcpy(&v.taken, w, 7 * 8);
  std::memcpy(out, &v, (size_t)v.struct_size);      // never more than the caller's struct holds
  return IEM_OK;
}

/* ---- the starting point: least-squares multipliers, the warm-start projection and its barrier parameter (csrc/iem_init_device.h) ---- */
struct iem_init {
  iem_barrier *b = nullptr;            // the object whose bounds, flags and grid it uses (borrowed)
  iem_init_opts_t opt;
  double *d_blk = nullptr;             // the own block: 16 words, then the slot of ynorm's bits and a word that stays +0.0 (the slot's seed)
};

namespace {
// InitArgs of csrc/iem_init_device.h
struct InitArgsH {
  const double *xl, *xu, *rl, *ru, *ceq;
  const unsigned char *fx, *fc;
  double *x, *s, *y, *zL, *zU, *vL, *vU;
  const double *r;
  const double *sol;
  double *sigma, *dcon, *rhs;
  unsigned long long *slot;
  const double *w;
  double *mblk;
  double *blk;
  double y_max, push, frac, z_push, z_max, y_clip, mu_factor, cap;
  double mu_init, mu_floor, tau_min;
  long long on_reject, nz;
  long long nvar, n;
};
InitArgsH init_args(const iem_init *q) {
  const iem_barrier *b = q->b;
  InitArgsH A;
  std::memset(&A, 0, sizeof A);
  A.xl = b->d_bounds; A.xu = A.xl + b->nvar; A.rl = A.xu + b->nvar; A.ru = A.rl + b->ncon; A.ceq = A.ru + b->ncon;
  A.fx = b->d_flags; A.fc = A.fx + b->nvar;
  A.blk = q->d_blk; A.slot = (unsigned long long *)(q->d_blk + 16);
  A.y_max = q->opt.y_max; A.on_reject = (long long)q->opt.on_reject;
  A.push = q->opt.warm_push; A.frac = q->opt.warm_frac; A.z_push = q->opt.warm_z_push; A.z_max = q->opt.warm_z_max; A.y_clip = q->opt.warm_y_max;
  A.mu_factor = q->opt.mu_factor; A.cap = q->opt.mu_cap;
  A.nz = (long long)(b->n_xl + b->n_xu + b->n_sl + b->n_su);
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon);
  return A;
}
int init_object(iem_model *m) {
  iem_model::InitObject &o = m->init;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = object_source(kInitSource, true, src);
  if (rc) return rc;
  KernelSlot slots[6] = {KernelSlot{"init_ls_terms", &o.ls_terms}, KernelSlot{"init_ls_norm", &o.ls_norm}, KernelSlot{"init_ls_apply", &o.ls_apply},
                         KernelSlot{"init_warm", &o.warm}, KernelSlot{"init_mu", &o.mu}, KernelSlot{"init_reset", &o.reset}};
  return load_object(m, src, slots, 6, &o.mod);
}
int init_opts(const iem_init_opts_t *in, iem_init_opts_t *out) {
  // Ipopt's constr_mult_init_max; its initialiser's y = 0 on rejection; warm_start_bound_push, _bound_frac, _mult_bound_push, _mult_init_max
  iem_init_opts_t v = {sizeof v, 1e3, 0, 1e-3, 1e-3, 1e-3, 1e6, 1e6, 1.0, 0.0};
  if (in) {
    if (in->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_init_create: set struct_size to sizeof(iem_init_opts_t) before the call");
    std::memcpy(&v, in, (size_t)std::min<uint64_t>(in->struct_size, sizeof v));      // (fields a shorter struct does not have keep their defaults)
    v.struct_size = sizeof v;
  }
  for (double f : {v.y_max, v.warm_push, v.warm_frac, v.warm_z_push, v.warm_z_max, v.warm_y_max, v.mu_factor, v.mu_cap})
    if (!std::isfinite(f)) return fail(IEM_E_ARG, "iem_init_create: every option must be finite");
  if (!(v.y_max >= 0.0)) return fail(IEM_E_ARG, "iem_init_create: y_max must not be negative");
  if (v.on_reject != 0 && v.on_reject != 1) return fail(IEM_E_ARG, "iem_init_create: on_reject must be 0 (write +0.0) or 1 (keep y)");
  if (!(v.warm_push > 0.0)) return fail(IEM_E_ARG, "iem_init_create: warm_push must be positive");
  if (!(v.warm_frac > 0.0) || !(v.warm_frac <= 0.5)) return fail(IEM_E_ARG, "iem_init_create: warm_frac must lie in (0, 0.5]");
  if (!(v.warm_z_push > 0.0)) return fail(IEM_E_ARG, "iem_init_create: warm_z_push must be positive");
  if (!(v.warm_z_max >= v.warm_z_push)) return fail(IEM_E_ARG, "iem_init_create: warm_z_max must be at least warm_z_push");
  if (!(v.warm_y_max > 0.0)) return fail(IEM_E_ARG, "iem_init_create: warm_y_max must be positive");
  if (!(v.mu_factor > 0.0)) return fail(IEM_E_ARG, "iem_init_create: mu_factor must be positive");
  if (!(v.mu_cap >= 0.0)) return fail(IEM_E_ARG, "iem_init_create: mu_cap must not be negative");
  *out = v;
  return IEM_OK;
}
}  // namespace

int iem_init_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = object_source(kInitSource, true, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_init_destroy(iem_init *q) {
  if (!q) return IEM_OK;
  DevGuard dg_(q->b->m->device);
  if (q->d_blk) hipFree(q->d_blk);
  delete q;
  return IEM_OK;
}

int iem_init_create(iem_barrier *b, const iem_init_opts_t *opts, iem_init **out) {
  if (!b || !out) return fail(IEM_E_ARG, "null argument");
  iem_init_opts_t opt;
  {
    int rc = init_opts(opts, &opt);
    if (rc) return rc;
  }
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  {
    int rc = init_object(m);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_init *q) const { iem_init_destroy(q); } };      // (a failed create frees what it had allocated)
  std::unique_ptr<iem_init, Drop> q(new iem_init);
  q->b = b;
  q->opt = opt;
  HIP_TRY(hipMalloc((void **)&q->d_blk, 18 * 8));
  HIP_TRY(hipMemset(q->d_blk, 0, 18 * 8));
  *out = q.release();
  return IEM_OK;
}

int iem_init_reset(iem_init *q) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  iem_model *m = q->b->m;
  DevGuard dg_(m->device);
  InitArgsH A = init_args(q);
  return kkt_launch_raw(m, m->init.reset, &A, sizeof A, 1, 64);
}

int iem_init_ls_terms(iem_init *q, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU, const double *d_r,
                      double *d_sigma, double *d_dcon, double *d_rhs) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->b;
  if ((b->nvar && (!d_zL || !d_zU || !d_r || !d_sigma)) || (b->ncon && (!d_y || !d_dcon)) || (b->n_ineq && (!d_vL || !d_vU)) || !d_rhs)
    return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  InitArgsH A = init_args(q);
  A.y = (double *)d_y; A.zL = (double *)d_zL; A.zU = (double *)d_zU; A.vL = (double *)d_vL; A.vU = (double *)d_vU;
  A.r = d_r; A.sigma = d_sigma; A.dcon = d_dcon; A.rhs = d_rhs;
  return kkt_launch_raw(m, m->init.ls_terms, &A, sizeof A, b->n_wg, 256);
}

int iem_init_ls_apply(iem_init *q, const double *d_sol, double *d_y) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->b;
  if (!d_sol || (b->ncon && !d_y)) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  InitArgsH A = init_args(q);
  A.sol = d_sol; A.y = d_y;
  // the seed: the maximum starts from the bits of +0.0 (a device-to-device copy is a capturable node, as in iem_barrier_step); without rows it stays there
  HIP_TRY(hipMemcpyAsync(A.slot, q->d_blk + 17, 8, hipMemcpyDeviceToDevice, m->stream));
  if (b->ncon) {
    int rc = kkt_launch_raw(m, m->init.ls_norm, &A, sizeof A, b->n_wg, 256);
    if (rc) return rc;
  }
  return kkt_launch_raw(m, m->init.ls_apply, &A, sizeof A, b->n_wg, 256);
}

int iem_init_warm(iem_init *q, double *d_x, double *d_s, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->b;
  if (barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU)) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  InitArgsH A = init_args(q);
  A.x = d_x; A.s = d_s; A.y = d_y; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU;
  return kkt_launch_raw(m, m->init.warm, &A, sizeof A, b->n_wg, 256);
}

int iem_init_mu(iem_init *q, const double *d_out12, iem_mu *p) {
  if (!q || !d_out12 || !p) return fail(IEM_E_ARG, "null argument");
  if (p->b != q->b) return fail(IEM_E_ARG, "iem_init_mu: the iem_mu object belongs to another barrier object");
  iem_model *m = q->b->m;
  DevGuard dg_(m->device);
  InitArgsH A = init_args(q);
  A.w = d_out12; A.mblk = p->d_blk;
  A.mu_init = p->opt.mu_init; A.mu_floor = p->opt.mu_floor; A.tau_min = p->opt.tau_min;
  if (A.cap == 0.0) A.cap = p->opt.mu_init;
  return kkt_launch_raw(m, m->init.mu, &A, sizeof A, 1, 64);
}

int iem_init_device(const iem_init *q, double **d_block) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  if (d_block) *d_block = q->d_blk;
  return IEM_OK;
}

int iem_init_state(iem_init *q, iem_init_state_t *out) {
  if (!q || !out) return fail(IEM_E_ARG, "null argument");
  if (out->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_init_state: set struct_size to sizeof(iem_init_state_t) before the call");
  iem_model *m = q->b->m;
  DevGuard dg_(m->device);
  uint64_t w[16];
  HIP_TRY(hipMemcpyAsync(w, q->d_blk, sizeof w, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  iem_init_state_t v;
  static_assert(sizeof v == 7 * 8, "iem_init_state_t: struct_size, then words 0-5 of the own block");
  v.struct_size = std::min<uint64_t>(out->struct_size, sizeof v);
  std::memcpy(&v.ynorm, w, 6 * 8);
  std::memcpy(out, &v, (size_t)v.struct_size);      // never more than the caller's struct holds
  return IEM_OK;
}

/* ---- the stopping test and the kept iterate (csrc/iem_conv_device.h) ---- */
struct iem_conv {
  iem_mu *p = nullptr;                 // the object whose barrier object, grid, tol, s_max, mu_floor and block it uses (borrowed)
  iem_conv_opts_t opt;
  double *d_blk = nullptr;             // the own block: 24 words, then the slots of xmax, rel, dymax and two words that stay +0.0 (the slots' seed)
  double *d_kept = nullptr;            // the kept point: x | s | y | zL | zU | vL | vU (3 nvar + 4 ncon doubles)
};

namespace {
constexpr int kConvWords = 24, kConvAlloc = kConvWords + 5;
// ConvArgs of csrc/iem_conv_device.h
struct ConvArgsH {
  const unsigned char *fx, *fc;
  double *x, *s, *y, *zL, *zU, *vL, *vU;
  double *kx, *ks, *ky, *kzL, *kzU, *kvL, *kvU;
  const double *sol, *ds;
  const double *w, *f;
  const double *mblk;
  double *blk;
  unsigned long long *slot;
  double tol, s_max, mu_floor;
  double dual_inf_tol, constr_viol_tol, compl_inf_tol;
  double acceptable_tol, acceptable_dual_inf_tol, acceptable_constr_viol_tol, acceptable_compl_inf_tol, acceptable_obj_change_tol;
  double diverging_iterates_tol, tiny_step_tol, tiny_step_y_tol;
  long long acceptable_iter, max_iter;
  long long ncon, nz;
  long long nvar, n;
};
void conv_kept(const iem_conv *q, double *out[7]) {
  const iem_barrier *b = q->p->b;
  const int64_t sizes[7] = {b->nvar, b->ncon, b->ncon, b->nvar, b->nvar, b->ncon, b->ncon};
  double *at = q->d_kept;
  for (int k = 0; k < 7; ++k) { out[k] = at; at += sizes[k]; }
}
ConvArgsH conv_args(const iem_conv *q) {
  const iem_mu *p = q->p;
  const iem_barrier *b = p->b;
  const iem_conv_opts_t &o = q->opt;
  ConvArgsH A;
  std::memset(&A, 0, sizeof A);
  A.fx = b->d_flags; A.fc = A.fx + b->nvar;
  double *k[7];
  conv_kept(q, k);
  A.kx = k[0]; A.ks = k[1]; A.ky = k[2]; A.kzL = k[3]; A.kzU = k[4]; A.kvL = k[5]; A.kvU = k[6];
  A.mblk = p->d_blk;
  A.blk = q->d_blk; A.slot = (unsigned long long *)(q->d_blk + kConvWords);
  A.tol = p->opt.tol; A.s_max = p->opt.s_max; A.mu_floor = p->opt.mu_floor;
  A.dual_inf_tol = o.dual_inf_tol; A.constr_viol_tol = o.constr_viol_tol; A.compl_inf_tol = o.compl_inf_tol;
  A.acceptable_tol = o.acceptable_tol; A.acceptable_dual_inf_tol = o.acceptable_dual_inf_tol; A.acceptable_constr_viol_tol = o.acceptable_constr_viol_tol;
  A.acceptable_compl_inf_tol = o.acceptable_compl_inf_tol; A.acceptable_obj_change_tol = o.acceptable_obj_change_tol;
  A.diverging_iterates_tol = o.diverging_iterates_tol; A.tiny_step_tol = o.tiny_step_tol; A.tiny_step_y_tol = o.tiny_step_y_tol;
  A.acceptable_iter = (long long)o.acceptable_iter; A.max_iter = (long long)o.max_iter;
  A.ncon = (long long)b->ncon; A.nz = (long long)(b->n_xl + b->n_xu + b->n_sl + b->n_su);
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon);
  return A;
}
void conv_set_state(ConvArgsH &A, const double *x, const double *s, const double *y, const double *zL, const double *zU, const double *vL, const double *vU) {
  A.x = (double *)x; A.s = (double *)s; A.y = (double *)y; A.zL = (double *)zL; A.zU = (double *)zU; A.vL = (double *)vL; A.vU = (double *)vU;
}
int conv_object(iem_model *m) {
  iem_model::ConvObject &o = m->conv;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = object_source(kConvSource, true, src);
  if (rc) return rc;
  KernelSlot slots[7] = {KernelSlot{"conv_xmax", &o.xmax}, KernelSlot{"conv_decide", &o.decide}, KernelSlot{"conv_stepmax", &o.stepmax}, KernelSlot{"conv_step_decide", &o.step_decide},
                         KernelSlot{"conv_keep", &o.keep}, KernelSlot{"conv_restore", &o.restore}, KernelSlot{"conv_reset", &o.reset}};
  return load_object(m, src, slots, 7, &o.mod);
}
int conv_opts(const iem_conv_opts_t *in, iem_conv_opts_t *out) {
  // Ipopt's dual_inf_tol, constr_viol_tol, compl_inf_tol, acceptable_tol, acceptable_iter, acceptable_dual_inf_tol, acceptable_constr_viol_tol,
  // acceptable_compl_inf_tol, acceptable_obj_change_tol, max_iter, diverging_iterates_tol, tiny_step_tol (10 machine epsilons), tiny_step_y_tol
  iem_conv_opts_t v = {sizeof v, 1.0, 1e-4, 1e-4, 1e-6, 15, 1e10, 1e-2, 1e-2, 1e20, 3000, 1e20, 10.0 * std::numeric_limits<double>::epsilon(), 1e-2};
  if (in) {
    if (in->struct_size != sizeof v) return fail(IEM_E_ARG, "iem_conv_create: set struct_size to sizeof(iem_conv_opts_t) before the call");
    v = *in;
  }
  const struct { const char *name; double value; } tols[] = {
      {"dual_inf_tol", v.dual_inf_tol}, {"constr_viol_tol", v.constr_viol_tol}, {"compl_inf_tol", v.compl_inf_tol}, {"acceptable_tol", v.acceptable_tol},
      {"acceptable_dual_inf_tol", v.acceptable_dual_inf_tol}, {"acceptable_constr_viol_tol", v.acceptable_constr_viol_tol},
      {"acceptable_compl_inf_tol", v.acceptable_compl_inf_tol}, {"acceptable_obj_change_tol", v.acceptable_obj_change_tol},
      {"diverging_iterates_tol", v.diverging_iterates_tol}, {"tiny_step_tol", v.tiny_step_tol}, {"tiny_step_y_tol", v.tiny_step_y_tol}};
  for (const auto &t : tols)
    if (!(t.value > 0.0)) return fail(IEM_E_ARG, std::string("iem_conv_create: ") + t.name + " must be positive (+inf switches the test off)");
  if (v.acceptable_iter < 0) return fail(IEM_E_ARG, "iem_conv_create: acceptable_iter must not be negative");
  if (v.max_iter < 0) return fail(IEM_E_ARG, "iem_conv_create: max_iter must not be negative");
  *out = v;
  return IEM_OK;
}
}  // namespace

int iem_conv_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = object_source(kConvSource, true, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_conv_destroy(iem_conv *q) {
  if (!q) return IEM_OK;
  DevGuard dg_(q->p->b->m->device);
  if (q->d_blk) hipFree(q->d_blk);
  if (q->d_kept) hipFree(q->d_kept);
  delete q;
  return IEM_OK;
}

int iem_conv_create(iem_mu *p, const iem_conv_opts_t *opts, iem_conv **out) {
  if (!p || !out) return fail(IEM_E_ARG, "null argument");
  iem_conv_opts_t opt;
  {
    int rc = conv_opts(opts, &opt);
    if (rc) return rc;
  }
  const iem_barrier *b = p->b;
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  {
    int rc = conv_object(m);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_conv *q) const { iem_conv_destroy(q); } };      // (a failed create frees what it had allocated)
  std::unique_ptr<iem_conv, Drop> q(new iem_conv);
  q->p = p;
  q->opt = opt;
  const size_t n_kept = (size_t)std::max<int64_t>(1, 3 * b->nvar + 4 * b->ncon);
  HIP_TRY(hipMalloc((void **)&q->d_blk, kConvAlloc * 8));
  HIP_TRY(hipMemset(q->d_blk, 0, kConvAlloc * 8));
  HIP_TRY(hipMalloc((void **)&q->d_kept, n_kept * 8));
  HIP_TRY(hipMemset(q->d_kept, 0, n_kept * 8));
  *out = q.release();
  return IEM_OK;
}

int iem_conv_reset(iem_conv *q) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  iem_model *m = q->p->b->m;
  DevGuard dg_(m->device);
  ConvArgsH A = conv_args(q);
  return kkt_launch_raw(m, m->conv.reset, &A, sizeof A, 1, 64);
}

int iem_conv_check(iem_conv *q, const double *d_out12, const double *d_f, const double *d_x) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->p->b;
  if (!d_out12 || !d_f || (b->nvar && !d_x)) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  ConvArgsH A = conv_args(q);
  A.w = d_out12; A.f = d_f; A.x = (double *)d_x;
  // the seed: the maximum starts from the bits of +0.0 (a device-to-device copy is a capturable node, as in iem_init_ls_apply)
  HIP_TRY(hipMemcpyAsync(A.slot, q->d_blk + kConvWords + 3, 8, hipMemcpyDeviceToDevice, m->stream));
  int rc = kkt_launch_raw(m, m->conv.xmax, &A, sizeof A, b->n_wg, 256);
  if (rc) return rc;
  return kkt_launch_raw(m, m->conv.decide, &A, sizeof A, 1, 64);
}

int iem_conv_keep(iem_conv *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->p->b;
  if (barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU)) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  ConvArgsH A = conv_args(q);
  conv_set_state(A, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU);
  return kkt_launch_raw(m, m->conv.keep, &A, sizeof A, b->n_wg, 256);
}

int iem_conv_restore(iem_conv *q, double *d_x, double *d_s, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->p->b;
  if (barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU)) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  ConvArgsH A = conv_args(q);
  conv_set_state(A, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU);
  return kkt_launch_raw(m, m->conv.restore, &A, sizeof A, b->n_wg, 256);
}

int iem_conv_step(iem_conv *q, const double *d_x, const double *d_s, const double *d_sol, const double *d_ds) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = q->p->b;
  if (!d_sol || (b->nvar && !d_x) || (b->n_ineq && (!d_s || !d_ds))) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  ConvArgsH A = conv_args(q);
  A.x = (double *)d_x; A.s = (double *)d_s; A.sol = d_sol; A.ds = d_ds;
  HIP_TRY(hipMemcpyAsync(A.slot + 1, q->d_blk + kConvWords + 3, 16, hipMemcpyDeviceToDevice, m->stream));      // the seeds of rel and dymax
  int rc = kkt_launch_raw(m, m->conv.stepmax, &A, sizeof A, b->n_wg, 256);
  if (rc) return rc;
  return kkt_launch_raw(m, m->conv.step_decide, &A, sizeof A, 1, 64);
}

int iem_conv_kept(const iem_conv *q, double **d_x, double **d_s, double **d_y, double **d_zL, double **d_zU, double **d_vL, double **d_vU) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  double *k[7];
  conv_kept(q, k);
  double **outs[7] = {d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU};
  for (int i = 0; i < 7; ++i)
    if (outs[i]) *outs[i] = k[i];
  return IEM_OK;
}

int iem_conv_device(const iem_conv *q, double **d_block) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  if (d_block) *d_block = q->d_blk;
  return IEM_OK;
}

int iem_conv_state(iem_conv *q, iem_conv_state_t *out) {
  if (!q || !out) return fail(IEM_E_ARG, "null argument");
  if (out->struct_size != sizeof(iem_conv_state_t)) return fail(IEM_E_ARG, "iem_conv_state: set struct_size to sizeof(iem_conv_state_t) before the call");
  iem_model *m = q->p->b->m;
  DevGuard dg_(m->device);
  uint64_t w[kConvWords];
  HIP_TRY(hipMemcpyAsync(w, q->d_blk, sizeof w, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  static_assert(sizeof(iem_conv_state_t) == 20 * 8, "iem_conv_state_t: struct_size, then words 0-18 of the own block");
  std::memcpy(&out->status, w, 19 * 8);
  return IEM_OK;
}

/* ---- the restoration phase's barrier parameter: candidates' error, the rule, enter, the alpha_min trigger, the bound restoration (csrc/iem_rmu_device.h) ---- */
struct iem_rmu {
  iem_resto *q = nullptr;              // the restoration object it was created on (borrowed)
  iem_mu *par = nullptr;               // the restoration block: a genuine iem_mu object on the same barrier object (owned)
  const iem_mu *orig = nullptr;        // the ORIGINAL problem's iem_mu object (borrowed), or null
  iem_rmu_opts_t opt;
  double *d_blk = nullptr;             // the own block: 16 words | the read-back's staging: 40 words | the seed of iem_rmu_error: 32 words
};

namespace {
constexpr int kRmuWords = 16, kRmuStage = 40, kRmuOut = 32, kRmuAlloc = kRmuWords + kRmuStage + kRmuOut;
static_assert(IEM_RMU_K == 6, "csrc/iem_rmu_device.h: RMU_K");
// RmuArgs of csrc/iem_rmu_device.h
struct RmuArgsH {
  const double *xl, *xu, *rl, *ru, *ceq;
  const unsigned char *fx, *fc;
  const double *x, *s, *y, *zL, *zU, *vL, *vU;
  const double *r, *c;
  const double *p, *n_, *zp, *zn, *sR, *ws, *xR, *wx;
  double *out;
  const double *w;
  double *blk;
  double *mblk;
  const double *oblk;
  const double *rblk;
  double *ctl;
  double *ictl;
  double *alpha;
  double *red;
  const long long *tab;
  double kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max, gamma_alpha;
  double rho, mu_host;
  double gamma_theta, gamma_phi, delta, s_theta, s_phi;
  long long which;
  long long ncon, nzr;
  long long nvar, n, n_wg;
};
RmuArgsH rmu_args(const iem_rmu *rp) {
  const iem_resto *q = rp->q;
  const iem_barrier *b = q->s->b;
  const iem_rmu_opts_t &o = rp->opt;
  RmuArgsH A;
  std::memset(&A, 0, sizeof A);
  A.xl = b->d_bounds; A.xu = A.xl + b->nvar; A.rl = A.xu + b->nvar; A.ru = A.rl + b->ncon; A.ceq = A.ru + b->ncon;
  A.fx = b->d_flags; A.fc = A.fx + b->nvar;
  const double *v = q->d_vec;
  const int64_t m = b->ncon;
  A.p = v; A.n_ = v + m; A.zp = v + 2 * m; A.zn = v + 3 * m; A.sR = v + 10 * m; A.ws = v + 11 * m; A.xR = v + 12 * m; A.wx = A.xR + b->nvar;
  A.blk = rp->d_blk; A.mblk = rp->par->d_blk; A.oblk = rp->orig ? rp->orig->d_blk : nullptr; A.rblk = q->d_blk;
  A.ictl = q->inner->d_ctl;
  A.red = rp->par->d_red; A.tab = rp->par->d_tab;      // the restoration block's own partial sums: six columns, as iem_mu_error's
  A.kappa_eps = o.kappa_eps; A.kappa_mu = o.kappa_mu; A.tau_min = o.tau_min; A.tol = o.tol; A.mu_floor = o.mu_floor; A.s_max = o.s_max; A.gamma_alpha = o.gamma_alpha;
  A.rho = q->opt.rho;
  A.ncon = (long long)b->ncon; A.nzr = (long long)(b->n_xl + b->n_xu + b->n_sl + b->n_su + 2 * b->ncon);
  A.nvar = (long long)b->nvar; A.n = (long long)(b->nvar + b->ncon); A.n_wg = (long long)b->n_wg;
  return A;
}
int rmu_object(iem_model *m) {
  iem_model::RmuObject &o = m->rmu;
  if (o.mod) return IEM_OK;
  std::string src;
  int rc = object_source(kRmuSource, true, src);
  if (rc) return rc;
  KernelSlot slots[5] = {KernelSlot{"rmu_error", &o.error}, KernelSlot{"rmu_enter", &o.enter}, KernelSlot{"rmu_update", &o.update}, KernelSlot{"rmu_trigger", &o.trigger},
                         KernelSlot{"rmu_gather", &o.gather}};
  return load_object(m, src, slots, 5, &o.mod);
}
int rmu_opts(const iem_rmu_opts_t *in, iem_rmu_opts_t *out) {
  iem_rmu_opts_t v = {sizeof v, 10.0, 0.2, 0.99, 1e-8, 1e-11, 100.0, 0.05};      // Ipopt's barrier_tol_factor, mu_linear_decrease_factor, tau_min, tol; the floor; s_max; alpha_min_frac
  if (in) {
    if (in->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_rmu_create: set struct_size to sizeof(iem_rmu_opts_t) before the call");
    std::memcpy(&v, in, (size_t)std::min<uint64_t>(in->struct_size, sizeof v));      // (fields a shorter struct does not have keep their defaults)
    v.struct_size = sizeof v;
  }
  const struct { const char *name; double value; bool unit; } rows[] = {
      {"kappa_eps", v.kappa_eps, false}, {"kappa_mu", v.kappa_mu, true}, {"tau_min", v.tau_min, true}, {"tol", v.tol, false},
      {"mu_floor", v.mu_floor, false}, {"s_max", v.s_max, false}, {"gamma_alpha", v.gamma_alpha, true}};
  for (const auto &r : rows) {
    if (!std::isfinite(r.value) || !(r.value > 0.0)) return fail(IEM_E_ARG, std::string("iem_rmu_create: ") + r.name + " must be positive and finite");
    if (r.unit && !(r.value < 1.0)) return fail(IEM_E_ARG, std::string("iem_rmu_create: ") + r.name + " must lie in (0, 1)");
  }
  *out = v;
  return IEM_OK;
}
}  // namespace

int iem_rmu_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = object_source(kRmuSource, true, s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_resto_mu_source(char **out_src, uint64_t *out_key) {
  std::string s;
  const int rc = resto_mu_source(s);
  return rc ? rc : emit_out(s, out_src, out_key);
}

int iem_rmu_destroy(iem_rmu *rp) {
  if (!rp) return IEM_OK;
  iem_resto *q = rp->q;
  DevGuard dg_(q->s->b->m->device);
  if (rp->par) {
    // whoever still reads the restoration block lets go of it: the iem_resto object and its inner search
    if (q->mu_blk == rp->par->d_blk) { q->mu_blk = nullptr; q->mu_orig_blk = nullptr; }
    if (q->inner->mu_blk == rp->par->d_blk) q->inner->mu_blk = nullptr;
    iem_mu_destroy(rp->par);
  }
  if (rp->d_blk) hipFree(rp->d_blk);
  delete rp;
  return IEM_OK;
}

int iem_rmu_create(iem_resto *q, const iem_mu *par_orig, const iem_rmu_opts_t *opts, iem_rmu **out) {
  if (!q || !out) return fail(IEM_E_ARG, "null argument");
  iem_rmu_opts_t opt;
  {
    int rc = rmu_opts(opts, &opt);
    if (rc) return rc;
  }
  iem_barrier *b = q->s->b;
  if (par_orig && par_orig->b != b) return fail(IEM_E_ARG, "iem_rmu_create: the original iem_mu object was created on another barrier object");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  {
    int rc = rmu_object(m);
    if (rc) return rc;
  }
  struct Drop { void operator()(iem_rmu *p) const { iem_rmu_destroy(p); } };      // (a failed create frees what it had allocated)
  std::unique_ptr<iem_rmu, Drop> rp(new iem_rmu);
  rp->q = q;
  rp->orig = par_orig;
  rp->opt = opt;
  {
    iem_mu_opts_t mo = {sizeof mo, 0.1, opt.kappa_eps, opt.kappa_mu, opt.tau_min, opt.tol, opt.mu_floor, opt.s_max};      // (mu_init: iem_rmu_enter writes the block before it is read)
    int rc = iem_mu_create(b, &mo, &rp->par);
    if (rc) return rc;
  }
  HIP_TRY(hipMalloc((void **)&rp->d_blk, kRmuAlloc * 8));
  double h[kRmuAlloc] = {};
  h[kRmuWords + kRmuStage + 8] = std::numeric_limits<double>::infinity();      // the seed: the minimum starts from +inf, everything else from +0.0
  HIP_TRY(hipMemcpy(rp->d_blk, h, sizeof h, hipMemcpyHostToDevice));
  *out = rp.release();
  return IEM_OK;
}

int iem_rmu_mu(const iem_rmu *rp, const iem_mu **out_par) {
  if (!rp || !out_par) return fail(IEM_E_ARG, "null argument");
  *out_par = rp->par;
  return IEM_OK;
}

int iem_resto_bind_mu(iem_resto *q, const iem_rmu *rp) {
  if (!q) return fail(IEM_E_ARG, "null argument");
  if (rp && rp->q != q) return fail(IEM_E_ARG, "iem_resto_bind_mu: the iem_rmu object was created on another iem_resto object");
  if (rp) {
    DevGuard dg_(q->s->b->m->device);
    int rc = resto_mu_object(q->s->b->m);
    if (rc) return rc;
  }
  q->mu_blk = rp ? rp->par->d_blk : nullptr;
  q->mu_orig_blk = rp && rp->orig ? rp->orig->d_blk : nullptr;
  return IEM_OK;
}

int iem_rmu_enter(iem_rmu *rp, const double *d_err, double mu_host) {
  if (!rp || !d_err) return fail(IEM_E_ARG, "null argument");
  iem_model *m = rp->q->s->b->m;
  DevGuard dg_(m->device);
  RmuArgsH A = rmu_args(rp);
  A.w = d_err; A.mu_host = mu_host;
  return kkt_launch_raw(m, m->rmu.enter, &A, sizeof A, 1, 64);
}

int iem_rmu_error(iem_rmu *rp, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
                  const double *d_r, const double *d_c, double *d_out) {
  if (!rp) return fail(IEM_E_ARG, "null argument");
  const iem_barrier *b = rp->q->s->b;
  if (barrier_state_missing(b, d_x, d_s, d_y, d_zL, d_zU, d_vL, d_vU) || (b->nvar && !d_r) || (b->ncon && !d_c) || !d_out) return fail(IEM_E_ARG, "null argument");
  iem_model *m = b->m;
  DevGuard dg_(m->device);
  RmuArgsH A = rmu_args(rp);
  A.x = d_x; A.s = d_s; A.y = d_y; A.zL = d_zL; A.zU = d_zU; A.vL = d_vL; A.vU = d_vU; A.r = d_r; A.c = d_c; A.out = d_out;
  // the seed: the maxima start from +0.0, the minimum from the bits of +inf (a device-to-device copy is a capturable node)
  HIP_TRY(hipMemcpyAsync(d_out, rp->d_blk + kRmuWords + kRmuStage, kRmuOut * 8, hipMemcpyDeviceToDevice, m->stream));
  return kkt_launch_raw(m, m->rmu.error, &A, sizeof A, b->n_wg, 256);
}

int iem_rmu_update(iem_rmu *rp, const double *d_out32) {
  if (!rp || !d_out32) return fail(IEM_E_ARG, "null argument");
  iem_model *m = rp->q->s->b->m;
  DevGuard dg_(m->device);
  RmuArgsH A = rmu_args(rp);
  A.w = d_out32;
  return kkt_launch_raw(m, m->rmu.update, &A, sizeof A, 1, 64);
}

int iem_rmu_trigger(iem_rmu *rp, int which, double *d_alpha) {
  if (which != 0 && which != 1) return fail(IEM_E_ARG, "iem_rmu_trigger: which must be 0 (the original search) or 1 (the inner search)");
  if (!rp || !d_alpha) return fail(IEM_E_ARG, "null argument");
  const iem_search *fs = which ? rp->q->inner : rp->q->s;
  iem_model *m = fs->b->m;
  DevGuard dg_(m->device);
  RmuArgsH A = rmu_args(rp);
  A.ctl = fs->d_ctl; A.alpha = d_alpha; A.which = which;
  A.gamma_theta = fs->opt.gamma_theta; A.gamma_phi = fs->opt.gamma_phi; A.delta = fs->opt.delta; A.s_theta = fs->opt.s_theta; A.s_phi = fs->opt.s_phi;
  return kkt_launch_raw(m, m->rmu.trigger, &A, sizeof A, 1, 64);
}

int iem_rmu_device(const iem_rmu *rp, double **d_block) {
  if (!rp) return fail(IEM_E_ARG, "null argument");
  if (d_block) *d_block = rp->d_blk;
  return IEM_OK;
}

int iem_rmu_state(iem_rmu *rp, iem_rmu_state_t *out) {
  if (!rp || !out) return fail(IEM_E_ARG, "null argument");
  if (out->struct_size < sizeof(uint64_t)) return fail(IEM_E_ARG, "iem_rmu_state: set struct_size to sizeof(iem_rmu_state_t) before the call");
  iem_model *m = rp->q->s->b->m;
  DevGuard dg_(m->device);
  RmuArgsH A = rmu_args(rp);
  A.out = rp->d_blk + kRmuWords;
  int rc = kkt_launch_raw(m, m->rmu.gather, &A, sizeof A, 1, 64);
  if (rc) return rc;
  uint64_t w[kRmuStage];
  HIP_TRY(hipMemcpyAsync(w, rp->d_blk + kRmuWords, sizeof w, hipMemcpyDeviceToHost, m->stream));      // the ONE copy: three blocks
  HIP_TRY(hipStreamSynchronize(m->stream));
  iem_rmu_state_t v;
  static_assert(sizeof v == 28 * 8, "iem_rmu_state_t: struct_size, words 0-10 of the own block, 0-11 of the restoration block, 0-3 of the iem_resto block");
  v.struct_size = std::min<uint64_t>(out->struct_size, sizeof v);
  std::memcpy(&v.status, w, 11 * 8);
  std::memcpy(&v.mu, w + 16, 12 * 8);
  std::memcpy(&v.resto_state, w + 32, 4 * 8);
  std::memcpy(out, &v, (size_t)v.struct_size);      // never more than the caller's struct holds
  return IEM_OK;
}

int iem_tuner_choice(iem_model *m, int kind, const double *d_vals, int *out_choice) {
  if (!m || !out_choice || kind < 0 || kind > 1) return fail(IEM_E_ARG, "bad argument");
  *out_choice = -1;
  if (m->alt.mod)
    for (auto &t : m->tune[kind].slot)
      if (t.out == d_vals) *out_choice = t.choice;
  return IEM_OK;
}

int iem_tune(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_jac, double *d_hess) {
  if (!m || !d_x || (d_hess && !d_y)) return fail(IEM_E_ARG, "bad argument");
  if (!m->alt.mod) return IEM_OK;
  DevGuard dg_(m->device);
  // Per kind and variant, twice: six warm launches, then ten launches between ONE pair of events (the faster block counts) — the steady state of that
  // kernel into that buffer.  (Events around every single launch, as the implicit tuner of a running solve uses,
  // perturb a pipeline of un-synchronised launches, the large-batch object more than the default: measured
  // 0.112 ms where ten back-to-back launches take 0.090 — profiles/r02_ab_autotune.txt.)
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return fail(IEM_E_HIP, "hipEventCreate"); }
  int rc = IEM_OK;
  for (int which = 0; which < 2 && rc == IEM_OK; ++which) {
    double *out = which ? d_hess : d_jac;
    if (!out) continue;
    const int kind = which ? iem::KK_HESS : iem::KK_JAC;
    float ms[2] = {1e30f, 1e30f};
    for (int round = 0; round < 2 && rc == IEM_OK; ++round)   // default, large batch, default, large batch: the first blocks of a process run on a GPU that is still ramping up
    for (int v = 0; v < 2 && rc == IEM_OK; ++v) {
      LaunchHead h;
      h.x = d_x; h.y = d_y; h.out = out; h.w = obj_weight;
      auto go = [&]() { return launch_kind(m, v ? m->alt : m->code, kind, h); };
      for (int i = 0; i < 6 && rc == IEM_OK; ++i) rc = go();   // warm: the first launches of a code object run cold
      if (rc == IEM_OK && hipEventRecord(e0, m->stream) != hipSuccess) rc = fail(IEM_E_HIP, "hipEventRecord");
      for (int i = 0; i < 10 && rc == IEM_OK; ++i) rc = go();
      float t = 0.f;
      if (rc == IEM_OK && (hipEventRecord(e1, m->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                           hipEventElapsedTime(&t, e0, e1) != hipSuccess)) rc = fail(IEM_E_HIP, "event timing");
      ms[v] = std::min(ms[v], t);
      if (getenv("IEM_TUNER_LOG")) fprintf(stderr, "iem tuner (iem_tune): kind %d round %d variant %d block %.4f ms per launch\n", kind, round, v, t / 10);
    }
    if (rc != IEM_OK) break;
    iem_model::Tune &T = tune_slot(m, which, out);
    T.calls = IEM_TUNE_CALLS;
    T.choice = ms[1] < 0.98f * ms[0] ? 1 : 0;
    if (getenv("IEM_TUNER_LOG"))
      fprintf(stderr, "iem tuner (iem_tune): kind %d buffer %p: default %.4f ms, large batch %.4f ms -> %s\n", kind, (const void *)out,
              ms[0] / 10, ms[1] / 10, T.choice ? "large batch" : "default");
  }
  hipEventDestroy(e0); hipEventDestroy(e1);
  if (rc == IEM_OK) HIP_TRY(hipStreamSynchronize(m->stream));
  return rc;
}

int iem_time_kernels(iem_model *m, const double *d_x, const double *d_y, double *d_jac, double *d_hess, int iters,
                     double *h_ms_jac, double *h_ms_hess) {
  if (!m || iters <= 0) return fail(IEM_E_ARG, "bad argument");
  DevGuard dg_(m->device);
  // Average launch duration in steady state: the jac/hess pair is enqueued `iters` times back to
  // back (as a solver loop does) with an event pair around EVERY launch, all on the launch
  // stream, and nothing synchronises until the end — the same quantity rocprofv3
  // --kernel-trace --stats reports as the kernel's average duration.
  std::vector<hipEvent_t> ev((size_t)iters * 4);
  for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
  int rc = IEM_OK;
  for (int w = 0; w < 3 && !rc; ++w) {   // warm-up pairs
    rc = iem_jac_coord(m, d_x, d_jac);
    if (!rc) rc = iem_hess_coord(m, d_x, d_y, 1.0, d_hess);
  }
  for (int it = 0; it < iters && !rc; ++it) {
    HIP_TRY(hipEventRecord(ev[4 * it + 0], m->stream));
    rc = iem_jac_coord(m, d_x, d_jac);
    HIP_TRY(hipEventRecord(ev[4 * it + 1], m->stream));
    HIP_TRY(hipEventRecord(ev[4 * it + 2], m->stream));
    if (!rc) rc = iem_hess_coord(m, d_x, d_y, 1.0, d_hess);
    HIP_TRY(hipEventRecord(ev[4 * it + 3], m->stream));
  }
  HIP_TRY(hipStreamSynchronize(m->stream));
  double tj = 0.0, th = 0.0;
  for (int it = 0; it < iters && !rc; ++it) {
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, ev[4 * it + 0], ev[4 * it + 1]));
    HIP_TRY(hipEventElapsedTime(&b, ev[4 * it + 2], ev[4 * it + 3]));
    tj += a; th += b;
  }
  for (auto &e : ev) hipEventDestroy(e);
  if (rc) return rc;
  *h_ms_jac = tj / iters;
  *h_ms_hess = th / iters;
  return IEM_OK;
}

}  // extern "C"
