// rmu_calls_check.cpp — sanitizer harness for the host side of the restoration phase's barrier parameter (iem_rmu_*, iem_resto_bind_mu,
// include/iem.h): every entry point's null refusals, each row of the option range table (every option at 0, −1, ±inf and a NaN; the
// three that must stay below 1 at 1 and 1.5; a struct_size below 8), which iem_rmu_create refuses BEFORE it touches the iem_resto
// object or a device — both source calls (text, key, free; the bound variant's edits all match, or the call fails) — and, where a
// device and a blob are there, the chain create → barrier → search → resto → mu → rmu → bind → enter → state → unbind → destroy.
// Without a device the chain ends at iem_create with its error and the rest is reported as not run.  Build with
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -w -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -Iinclude tools/rmu_calls_check.cpp infiniteexamodels.jl_amd/csrc/iem_api.cpp \
//       infiniteexamodels.jl_amd/csrc/iem_codegen.cpp -L/opt/rocm/lib -lamdhip64 -lhiprtc -ldl -Wl,-rpath,/opt/rocm/lib -o /tmp/rmu_calls_check
// (csrc/Makefile writes the *_h.inc files the first source includes) and run it, with a blob file (ExaCore.to_blob()) for the chain.
// Exit status 0: every call answered as expected.
#include "iem.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
#include <string>
#include <vector>

static uint64_t fnv1a64(const char *s) {
  uint64_t h = 1469598103934665603ull;
  for (; *s; ++s) { h ^= (unsigned char)*s; h *= 1099511628211ull; }
  return h;
}

static iem_rmu_opts_t defaults() {
  iem_rmu_opts_t o = {sizeof o, 10.0, 0.2, 0.99, 1e-8, 1e-11, 100.0, 0.05};
  return o;
}

int main(int argc, char **argv) {
  int bad = 0;
  auto expect = [&](const char *what, int rc, int want, const char *needle) {
    const std::string msg = rc == IEM_OK ? "" : iem_last_error();
    const bool ok = rc == want && (!needle || msg.find(needle) != std::string::npos);
    std::printf("%-58s rc %d  %s%s\n", what, rc, ok ? "ok" : "BAD: ", ok ? "" : msg.c_str());
    if (!ok) ++bad;
  };
  // null handles: refused before anything else
  iem_rmu *out = nullptr;
  iem_rmu_opts_t o = defaults();
  double *dp = nullptr;
  const iem_mu *par = nullptr;
  double alpha[2] = {};
  iem_rmu_state_t st;
  std::memset(&st, 0, sizeof st);
  st.struct_size = sizeof st;
  expect("iem_rmu_create(NULL, NULL, NULL, &out)", iem_rmu_create(nullptr, nullptr, nullptr, &out), IEM_E_ARG, "null");
  expect("iem_rmu_create(NULL, NULL, &opts, NULL)", iem_rmu_create(nullptr, nullptr, &o, nullptr), IEM_E_ARG, "null");
  expect("iem_rmu_destroy(NULL)", iem_rmu_destroy(nullptr), IEM_OK, nullptr);
  expect("iem_rmu_mu(NULL, &par)", iem_rmu_mu(nullptr, &par), IEM_E_ARG, "null");
  expect("iem_rmu_enter(NULL, ...)", iem_rmu_enter(nullptr, nullptr, 0.1), IEM_E_ARG, "null");
  expect("iem_rmu_error(NULL, ...)", iem_rmu_error(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), IEM_E_ARG, "null");
  expect("iem_rmu_update(NULL, NULL)", iem_rmu_update(nullptr, nullptr), IEM_E_ARG, "null");
  expect("iem_rmu_trigger(NULL, 0, alpha)", iem_rmu_trigger(nullptr, 0, alpha), IEM_E_ARG, "null");
  expect("iem_rmu_trigger(NULL, 2, alpha)", iem_rmu_trigger(nullptr, 2, alpha), IEM_E_ARG, "which");
  expect("iem_rmu_trigger(NULL, -1, alpha)", iem_rmu_trigger(nullptr, -1, alpha), IEM_E_ARG, "which");
  expect("iem_rmu_device(NULL, &p)", iem_rmu_device(nullptr, &dp), IEM_E_ARG, "null");
  expect("iem_rmu_state(NULL, &st)", iem_rmu_state(nullptr, &st), IEM_E_ARG, "null");
  expect("iem_resto_bind_mu(NULL, NULL)", iem_resto_bind_mu(nullptr, nullptr), IEM_E_ARG, "null");
  // the range table: refused before the iem_resto object is looked at (the handle below is never dereferenced)
  alignas(16) static unsigned char never_read[512];
  iem_resto *fake = reinterpret_cast<iem_resto *>(never_read);
  struct Field { const char *name; double iem_rmu_opts_t::*at; bool unit; };
  const Field fields[7] = {{"kappa_eps", &iem_rmu_opts_t::kappa_eps, false}, {"kappa_mu", &iem_rmu_opts_t::kappa_mu, true}, {"tau_min", &iem_rmu_opts_t::tau_min, true},
                           {"tol", &iem_rmu_opts_t::tol, false}, {"mu_floor", &iem_rmu_opts_t::mu_floor, false}, {"s_max", &iem_rmu_opts_t::s_max, false},
                           {"gamma_alpha", &iem_rmu_opts_t::gamma_alpha, true}};
  const double inf = std::numeric_limits<double>::infinity();
  const double bads[7] = {0.0, -1.0, -inf, inf, std::nan(""), 1.0, 1.5};
  for (const Field &f : fields)
    for (int k = 0; k < (f.unit ? 7 : 5); ++k) {
      o = defaults();
      o.*(f.at) = bads[k];
      expect((std::string("iem_rmu_create: ") + f.name + " = " + std::to_string(bads[k])).c_str(), iem_rmu_create(fake, nullptr, &o, &out), IEM_E_ARG, f.name);
    }
  for (uint64_t size : {(uint64_t)0, (uint64_t)4, (uint64_t)7}) {
    o = defaults(); o.struct_size = size;
    expect((std::string("iem_rmu_create: struct_size = ") + std::to_string(size)).c_str(), iem_rmu_create(fake, nullptr, &o, &out), IEM_E_ARG, "struct_size");
  }
  if (out) { std::printf("a refused create wrote its output\n"); ++bad; }
  // the two sources: text and key, freed
  uint64_t resto_key = 0;
  {
    char *src = nullptr;
    const int rc = iem_resto_source(&src, &resto_key);
    if (rc != IEM_OK || !src) ++bad;
    if (src) iem_free(src);
  }
  for (int which = 0; which < 2; ++which) {
    char *src = nullptr;
    uint64_t key = 0;
    const int rc = which ? iem_resto_mu_source(&src, &key) : iem_rmu_source(&src, &key);
    const bool ok = rc == IEM_OK && src && std::strncmp(src, "// iem-flags:", 13) == 0 && fnv1a64(src) == key && key != resto_key &&
                    std::strstr(src, which ? "A.mu_orig_blk ? A.mu_orig_blk[0] : A.mu" : "rmu_trigger") && (!which || !std::strstr(src, "A.zeta"));
    std::printf("%-58s rc %d  %zu bytes  key %016llx  %s\n", which ? "iem_resto_mu_source" : "iem_rmu_source", rc, src ? std::strlen(src) : (size_t)0, (unsigned long long)key,
                ok ? "ok" : "BAD");
    if (!ok) ++bad;
    if (src) iem_free(src);
  }
  expect("iem_rmu_source(NULL, NULL)", iem_rmu_source(nullptr, nullptr), IEM_OK, nullptr);
  expect("iem_resto_mu_source(NULL, NULL)", iem_resto_mu_source(nullptr, nullptr), IEM_OK, nullptr);
  // the chain, where a device is there
  if (argc > 1) {
    std::ifstream file(argv[1], std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
    iem_model *m = nullptr;
    const int rc = iem_create(b.data(), b.size(), 0, &m);
    if (rc != IEM_OK) {
      std::printf("iem_create: rc %d (%s): no device here, the chain create -> rmu -> destroy was NOT run\n", rc, iem_last_error());
    } else {
      iem_barrier *bar = nullptr;
      iem_search *fs = nullptr;
      iem_resto *q = nullptr;
      iem_mu *orig = nullptr;
      iem_rmu *rp = nullptr;
      expect("iem_barrier_create", iem_barrier_create(m, nullptr, nullptr, nullptr, nullptr, 1e-8, &bar), IEM_OK, nullptr);
      expect("iem_search_create", iem_search_create(bar, nullptr, &fs), IEM_OK, nullptr);
      expect("iem_resto_create", iem_resto_create(fs, nullptr, &q), IEM_OK, nullptr);
      expect("iem_mu_create", iem_mu_create(bar, nullptr, &orig), IEM_OK, nullptr);
      expect("iem_rmu_create(q, orig, NULL, &rp)", iem_rmu_create(q, orig, nullptr, &rp), IEM_OK, nullptr);
      expect("iem_rmu_mu", iem_rmu_mu(rp, &par), IEM_OK, nullptr);
      expect("iem_resto_bind_mu(q, rp)", iem_resto_bind_mu(q, rp), IEM_OK, nullptr);
      expect("iem_rmu_state", iem_rmu_state(rp, &st), IEM_OK, nullptr);
      st.struct_size = 4;
      expect("iem_rmu_state: struct_size = 4", iem_rmu_state(rp, &st), IEM_E_ARG, "struct_size");
      expect("iem_rmu_update(rp, NULL)", iem_rmu_update(rp, nullptr), IEM_E_ARG, "null");
      expect("iem_resto_bind_mu(q, NULL)", iem_resto_bind_mu(q, nullptr), IEM_OK, nullptr);
      expect("iem_rmu_destroy", iem_rmu_destroy(rp), IEM_OK, nullptr);
      expect("iem_mu_destroy", iem_mu_destroy(orig), IEM_OK, nullptr);
      expect("iem_resto_destroy", iem_resto_destroy(q), IEM_OK, nullptr);
      expect("iem_search_destroy", iem_search_destroy(fs), IEM_OK, nullptr);
      expect("iem_barrier_destroy", iem_barrier_destroy(bar), IEM_OK, nullptr);
      expect("iem_destroy", iem_destroy(m), IEM_OK, nullptr);
    }
  } else {
    std::printf("no blob given: the chain create -> rmu -> destroy was NOT run\n");
  }
  std::printf("%s\n", bad ? "FAILED" : "all restoration-parameter calls ok");
  return bad ? 1 : 0;
}
