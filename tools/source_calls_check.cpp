// source_calls_check.cpp — sanitizer harness for the source entry points (host only, no device): iem_fixed_source over the
// indices -1 .. 3, the four named *_source calls and iem_emit_source on one blob — for each of the generator's nine programs,
// selected through iem_set_option and reset afterwards, and for the six pairs of two program options at once, each refused with
// its message — everything they return freed.  Build with
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -w -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -Iinclude tools/source_calls_check.cpp infiniteexamodels.jl_amd/csrc/iem_api.cpp \
//       infiniteexamodels.jl_amd/csrc/iem_codegen.cpp -L/opt/rocm/lib -lamdhip64 -lhiprtc -ldl -Wl,-rpath,/opt/rocm/lib -o /tmp/source_calls_check
// and run it on a blob file (ExaCore.to_blob()).  Exit status 0: every call answered as expected.
#include "iem.h"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

static uint64_t fnv1a64(const char *s) {
  uint64_t h = 1469598103934665603ull;
  for (; *s; ++s) { h ^= (unsigned char)*s; h *= 1099511628211ull; }
  return h;
}

int main(int argc, char **argv) {
  int bad = 0;
  auto report = [&](const char *what, int rc, char *src, uint64_t key) {
    const bool ok = rc == IEM_OK && src && std::strncmp(src, "// iem-flags:", 13) == 0 && fnv1a64(src) == key;
    std::printf("%-28s rc %d  %7zu bytes  key %016llx  %s\n", what, rc, src ? std::strlen(src) : (size_t)0, (unsigned long long)key, ok ? "ok" : "BAD");
    if (!ok) ++bad;
    if (src) iem_free(src);
  };
  std::vector<std::string> listed;
  for (int i = -1; i <= 3; ++i) {
    const char *name = "(untouched)";
    char *src = nullptr;
    uint64_t key = 0;
    const int rc = iem_fixed_source(i, &name, &src, &key);
    if (i < 0 || i >= 3) {
      const bool ok = rc == IEM_E_ARG && !src && key == 0 && std::strcmp(name, "(untouched)") == 0;
      std::printf("iem_fixed_source(%d)         rc %d  %s\n", i, rc, ok ? "refused, nothing written" : "BAD");
      if (!ok) ++bad;
      continue;
    }
    listed.push_back(src ? src : "");
    report((std::string("iem_fixed_source(") + std::to_string(i) + ") " + name).c_str(), rc, src, key);
    if (iem_fixed_source(i, nullptr, nullptr, nullptr) != IEM_OK) ++bad;      // every output is optional
  }
  typedef int (*named_t)(char **, uint64_t *);
  const named_t named[3] = {iem_kkt_diag_source, iem_kkt_border_source, iem_barrier_source};
  const char *names[3] = {"iem_kkt_diag_source", "iem_kkt_border_source", "iem_barrier_source"};
  for (int i = 0; i < 3; ++i) {
    char *src = nullptr;
    uint64_t key = 0;
    const int rc = named[i](&src, &key);
    if (!src || listed.size() != 3 || listed[i] != src) { std::printf("%s differs from the listed source\n", names[i]); ++bad; }
    report(names[i], rc, src, key);
  }
  {
    char *src = nullptr;
    uint64_t key = 0;
    const int rc = iem_kkt_source(40, 0, 12, &src, &key);
    report("iem_kkt_source(40, 0, 12)", rc, src, key);
  }
  if (argc > 1) {
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    struct Opt { const char *name; int value; };
    const Opt programs[9] = {{"param_kinds", 0}, {"param_kinds", 1}, {"param_kinds", 2}, {"param_kinds", 3}, {"param_kinds", 4}, {"param_kinds", 5},
                             {"scaled_kinds", 1}, {"kkt_kinds", 1}, {"scaled_phase_kinds", 1}};
    std::vector<uint64_t> keys;
    for (const Opt &pg : programs) {
      char *src = nullptr;
      uint64_t key = 0;
      if (iem_set_option(pg.name, pg.value) != IEM_OK) ++bad;
      const int rc = iem_emit_source(b.data(), b.size(), &src, &key);
      if (iem_set_option(pg.name, 0) != IEM_OK) ++bad;
      for (uint64_t k : keys) if (k == key) { std::printf("%s=%d: the key of another program\n", pg.name, pg.value); ++bad; }
      keys.push_back(key);
      report((std::string("iem_emit_source ") + pg.name + "=" + std::to_string(pg.value)).c_str(), rc, src, key);
    }
    // two program options at once: refused with the message that names both, in the generator's order of precedence
    const char *pairs[6][2] = {{"scaled_phase_kinds", "param_kinds"}, {"scaled_phase_kinds", "scaled_kinds"}, {"scaled_phase_kinds", "kkt_kinds"},
                               {"scaled_kinds", "param_kinds"}, {"scaled_kinds", "kkt_kinds"}, {"kkt_kinds", "param_kinds"}};
    for (const auto &pr : pairs) {
      char *src = nullptr;
      uint64_t key = 0;
      if (iem_set_option(pr[0], 1) != IEM_OK || iem_set_option(pr[1], 1) != IEM_OK) ++bad;
      const int rc = iem_emit_source(b.data(), b.size(), &src, &key);
      const std::string want = std::string(pr[0]) + " and " + pr[1] + " name different programs: set one of them", got = iem_last_error();
      if (iem_set_option(pr[0], 0) != IEM_OK || iem_set_option(pr[1], 0) != IEM_OK) ++bad;
      const bool ok = rc != IEM_OK && !src && got == want;
      std::printf("%-18s + %-12s rc %d  %s\n", pr[0], pr[1], rc, ok ? "refused with its message" : ("BAD: " + got).c_str());
      if (!ok) ++bad;
      if (src) iem_free(src);
    }
  } else {
    std::printf("no blob given: iem_emit_source not called\n");
    ++bad;
  }
  std::printf("%s\n", bad ? "FAILED" : "all source calls ok");
  return bad ? 1 : 0;
}
