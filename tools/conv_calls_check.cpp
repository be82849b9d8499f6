// conv_calls_check.cpp — sanitizer harness for the host side of the stopping test (iem_conv_*, include/iem.h): every entry point's
// argument checks — null handles, each row of the option range table (every tolerance at 0, −1, −inf and a NaN; negative counts; a
// struct_size that is not the struct's), which iem_conv_create refuses BEFORE it touches the iem_mu object or a device — the source
// call (text, key, free), and, where a device and a blob are there, the chain create → barrier → mu → conv → state → destroy.
// Without a device the chain ends at iem_create with its error and the rest is reported as not run.  Build with
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -w -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -Iinclude tools/conv_calls_check.cpp infiniteexamodels.jl_amd/csrc/iem_api.cpp \
//       infiniteexamodels.jl_amd/csrc/iem_codegen.cpp -L/opt/rocm/lib -lamdhip64 -lhiprtc -ldl -Wl,-rpath,/opt/rocm/lib -o /tmp/conv_calls_check
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

static iem_conv_opts_t defaults() {
  iem_conv_opts_t o = {sizeof o, 1.0, 1e-4, 1e-4, 1e-6, 15, 1e10, 1e-2, 1e-2, 1e20, 3000, 1e20, 10.0 * std::numeric_limits<double>::epsilon(), 1e-2};
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
  iem_conv *out = nullptr;
  iem_conv_opts_t o = defaults();
  double *dp[7] = {};
  iem_conv_state_t st;
  std::memset(&st, 0, sizeof st);
  st.struct_size = sizeof st;
  expect("iem_conv_create(NULL, NULL, &out)", iem_conv_create(nullptr, nullptr, &out), IEM_E_ARG, "null");
  expect("iem_conv_create(NULL, &opts, NULL)", iem_conv_create(nullptr, &o, nullptr), IEM_E_ARG, "null");
  expect("iem_conv_destroy(NULL)", iem_conv_destroy(nullptr), IEM_OK, nullptr);
  expect("iem_conv_reset(NULL)", iem_conv_reset(nullptr), IEM_E_ARG, "null");
  expect("iem_conv_check(NULL, ...)", iem_conv_check(nullptr, nullptr, nullptr, nullptr), IEM_E_ARG, "null");
  expect("iem_conv_keep(NULL, ...)", iem_conv_keep(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), IEM_E_ARG, "null");
  expect("iem_conv_restore(NULL, ...)", iem_conv_restore(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), IEM_E_ARG, "null");
  expect("iem_conv_step(NULL, ...)", iem_conv_step(nullptr, nullptr, nullptr, nullptr, nullptr), IEM_E_ARG, "null");
  expect("iem_conv_kept(NULL, ...)", iem_conv_kept(nullptr, &dp[0], &dp[1], &dp[2], &dp[3], &dp[4], &dp[5], &dp[6]), IEM_E_ARG, "null");
  expect("iem_conv_device(NULL, &p)", iem_conv_device(nullptr, &dp[0]), IEM_E_ARG, "null");
  expect("iem_conv_state(NULL, &st)", iem_conv_state(nullptr, &st), IEM_E_ARG, "null");
  // the range table: refused before the iem_mu object is looked at (the handle below is never dereferenced)
  alignas(16) static unsigned char never_read[256];
  iem_mu *fake = reinterpret_cast<iem_mu *>(never_read);
  struct Field { const char *name; double iem_conv_opts_t::*at; };
  const Field fields[11] = {{"dual_inf_tol", &iem_conv_opts_t::dual_inf_tol}, {"constr_viol_tol", &iem_conv_opts_t::constr_viol_tol}, {"compl_inf_tol", &iem_conv_opts_t::compl_inf_tol},
                            {"acceptable_tol", &iem_conv_opts_t::acceptable_tol}, {"acceptable_dual_inf_tol", &iem_conv_opts_t::acceptable_dual_inf_tol},
                            {"acceptable_constr_viol_tol", &iem_conv_opts_t::acceptable_constr_viol_tol}, {"acceptable_compl_inf_tol", &iem_conv_opts_t::acceptable_compl_inf_tol},
                            {"acceptable_obj_change_tol", &iem_conv_opts_t::acceptable_obj_change_tol}, {"diverging_iterates_tol", &iem_conv_opts_t::diverging_iterates_tol},
                            {"tiny_step_tol", &iem_conv_opts_t::tiny_step_tol}, {"tiny_step_y_tol", &iem_conv_opts_t::tiny_step_y_tol}};
  const double bads[4] = {0.0, -1.0, -std::numeric_limits<double>::infinity(), std::nan("")};
  for (const Field &f : fields)
    for (double v : bads) {
      o = defaults();
      o.*(f.at) = v;
      expect((std::string("iem_conv_create: ") + f.name + " = " + std::to_string(v)).c_str(), iem_conv_create(fake, &o, &out), IEM_E_ARG, f.name);
    }
  o = defaults(); o.acceptable_iter = -1;
  expect("iem_conv_create: acceptable_iter = -1", iem_conv_create(fake, &o, &out), IEM_E_ARG, "acceptable_iter");
  o = defaults(); o.max_iter = -1;
  expect("iem_conv_create: max_iter = -1", iem_conv_create(fake, &o, &out), IEM_E_ARG, "max_iter");
  for (uint64_t size : {(uint64_t)0, (uint64_t)4, (uint64_t)(sizeof o - 8), (uint64_t)(sizeof o + 8)}) {
    o = defaults(); o.struct_size = size;
    expect((std::string("iem_conv_create: struct_size = ") + std::to_string(size)).c_str(), iem_conv_create(fake, &o, &out), IEM_E_ARG, "struct_size");
  }
  if (out) { std::printf("a refused create wrote its output\n"); ++bad; }
  // the source: text and key, freed
  {
    char *src = nullptr;
    uint64_t key = 0;
    const int rc = iem_conv_source(&src, &key);
    const bool ok = rc == IEM_OK && src && std::strncmp(src, "// iem-flags:", 13) == 0 && fnv1a64(src) == key && std::strstr(src, "conv_decide");
    std::printf("%-58s rc %d  %zu bytes  key %016llx  %s\n", "iem_conv_source", rc, src ? std::strlen(src) : (size_t)0, (unsigned long long)key, ok ? "ok" : "BAD");
    if (!ok) ++bad;
    if (src) iem_free(src);
  }
  // the chain, where a device is there
  if (argc > 1) {
    std::ifstream file(argv[1], std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
    iem_model *m = nullptr;
    const int rc = iem_create(b.data(), b.size(), 0, &m);
    if (rc != IEM_OK) {
      std::printf("iem_create: rc %d (%s): no device here, the chain create -> conv -> destroy was NOT run\n", rc, iem_last_error());
    } else {
      iem_barrier *bar = nullptr;
      iem_mu *par = nullptr;
      iem_conv *q = nullptr;
      expect("iem_barrier_create", iem_barrier_create(m, nullptr, nullptr, nullptr, nullptr, 1e-8, &bar), IEM_OK, nullptr);
      expect("iem_mu_create", iem_mu_create(bar, nullptr, &par), IEM_OK, nullptr);
      expect("iem_conv_create(par, NULL, &q)", iem_conv_create(par, nullptr, &q), IEM_OK, nullptr);
      expect("iem_conv_reset", iem_conv_reset(q), IEM_OK, nullptr);
      expect("iem_conv_state", iem_conv_state(q, &st), IEM_OK, nullptr);
      st.struct_size = 8;
      expect("iem_conv_state: struct_size = 8", iem_conv_state(q, &st), IEM_E_ARG, "struct_size");
      expect("iem_conv_check(q, NULL, ...)", iem_conv_check(q, nullptr, nullptr, nullptr), IEM_E_ARG, "null");
      expect("iem_conv_kept", iem_conv_kept(q, &dp[0], &dp[1], &dp[2], &dp[3], &dp[4], &dp[5], &dp[6]), IEM_OK, nullptr);
      expect("iem_conv_destroy", iem_conv_destroy(q), IEM_OK, nullptr);
      expect("iem_mu_destroy", iem_mu_destroy(par), IEM_OK, nullptr);
      expect("iem_barrier_destroy", iem_barrier_destroy(bar), IEM_OK, nullptr);
      expect("iem_destroy", iem_destroy(m), IEM_OK, nullptr);
    }
  } else {
    std::printf("no blob given: the chain create -> conv -> destroy was NOT run\n");
  }
  std::printf("%s\n", bad ? "FAILED" : "all stopping-test calls ok");
  return bad ? 1 : 0;
}
