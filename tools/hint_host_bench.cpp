// hint_host_bench -- wall time of the host ApplyHints (cld_hint_priors per
// document, the code apply_hints() runs for cld_detect_batch_ex) over a batch
// of HTML pages on T threads, each taking a contiguous share as apply_hints()
// does.  No GPU.  Driven by tools/hints_rate.py.
// usage: hint_host_bench LIB BUF OFFS THREADS REPEATS
//   BUF: the pages back to back; OFFS: uint64[n + 1]; one warm-up pass, then
//   REPEATS timed ones -> one JSON line (median and minimum, ms).
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>
typedef int (*fn_t)(const uint8_t*, size_t, int, const void*, int16_t*, uint32_t*);
static std::vector<uint8_t> slurp(const char* p) {
  FILE* f = fopen(p, "rb"); if (!f) { perror(p); exit(2); }
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> v(n); if (fread(v.data(), 1, n, f) != (size_t)n) exit(2); fclose(f); return v;
}
int main(int argc, char** argv) {
  if (argc < 6) return 2;
  void* h = dlopen(argv[1], RTLD_NOW); if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  fn_t fn = (fn_t)dlsym(h, "cld_hint_priors"); if (!fn) return 2;
  std::vector<uint8_t> buf = slurp(argv[2]), ob = slurp(argv[3]);
  const uint64_t* offs = (const uint64_t*)ob.data(); const size_t n = ob.size() / 8 - 1;
  const int T = atoi(argv[4]), R = atoi(argv[5]);
  std::vector<uint32_t> boosts(16 * n);
  std::vector<double> ms;
  for (int r = 0; r < R + 1; ++r) {
    auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back([&, t] {
      for (size_t i = n * t / T; i < n * (t + 1) / T; ++i) { int16_t p[14]; fn(buf.data() + offs[i], offs[i + 1] - offs[i], 0, nullptr, p, &boosts[16 * i]); }
    });
    for (auto& x : th) x.join();
    double d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r) ms.push_back(d);   // the first pass warms up (and loads the tables)
  }
  std::sort(ms.begin(), ms.end());
  size_t nz = 0; for (size_t i = 0; i < n; ++i) { bool a = false; for (int k = 0; k < 16; ++k) a |= boosts[16 * i + k] != 0; nz += a; }
  printf("{\"host_threads\": %d, \"docs\": %zu, \"bytes\": %zu, \"with_priors\": %zu, \"host_ms_median\": %.3f, \"host_ms_min\": %.3f}\n", T, n, buf.size(), nz, ms[ms.size() / 2], ms[0]);
  return 0;
}
