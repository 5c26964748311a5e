// What every program of tests/cpp/ (mirror drivers, bare-ABI benches, CPU references) shares, stated once: binary file I/O, float bit patterns, the ABI's
// die-on-error check, wall-clock summaries, the JSON fragments the Python side reads (tests/cpp_driver.py), the byte-wise row comparison and the host-side
// acceptance test and sort key the benches use as their baseline route.  Plain C++17 over include/lsm2d.h alone: no mirror type, no HIP header.
#pragma once
#include <lsm2d.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// ---- files: a whole file as a vector of T (exit 2 when it cannot be read); "-" as an argument means "absent"; a whole vector out, or exit 2
template <class T> inline std::vector<T> read_all(const char* path) {
  FILE* f = fopen(path, "rb"); if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END); long n = ftell(f) / (long) sizeof(T); fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t) n);
  if (n && fread(v.data(), sizeof(T), (size_t) n, f) != (size_t) n) exit(2);
  fclose(f); return v;
}
template <class T> inline std::vector<T> read_all(const std::string& path) { return read_all<T>(path.c_str()); }
template <class T> inline std::vector<T> read_all_or_empty(const char* arg) { return strcmp(arg, "-") ? read_all<T>(arg) : std::vector<T>(); }
template <class T> inline void write_all(const char* path, const T* p, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(p, sizeof(T), n, f) != n) { perror(path); exit(2); }
  fclose(f);
}
template <class T> inline void write_all(const std::string& path, const T* p, size_t n) { write_all(path.c_str(), p, n); }

// ---- float <-> bit pattern; the decimal string of one on a command line
inline uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, sizeof u); return u; }
inline float from_bits(uint32_t u) { float v; memcpy(&v, &u, sizeof v); return v; }
inline float from_bits_arg(const char* s) { return from_bits((uint32_t) strtoul(s, nullptr, 10)); }

// ---- the bare ABI: a negative status ends the program with the call's name and the context's last error
inline void must(int rc, const char* what, lsm2d_context* ctx) {
  if (rc < 0) { fprintf(stderr, "%s: %s %s\n", what, lsm2d_status_string(rc), lsm2d_last_error(ctx)); exit(1); }
}

// ---- timing: out = {median, minimum, maximum}, zeros for no samples.  The median of an even count is the mean of the middle pair; upper_middle = true asks
// for the upper middle element instead (what the occupancy and voxelize benches have always reported)
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline void summary(std::vector<double> t, double out[3], bool upper_middle = false) {
  if (t.empty()) { out[0] = out[1] = out[2] = 0.0; return; }
  std::sort(t.begin(), t.end());
  const size_t h = t.size() / 2;
  out[0] = (upper_middle || t.size() % 2) ? t[h] : 0.5 * (t[h - 1] + t[h]); out[1] = t.front(); out[2] = t.back();
}

// ---- JSON fragments: "name": [..]tail with integers or with floats as their bit patterns; the statistics triple tests/cpp_driver.stats_json mirrors
template <class V> inline void print_int_list(const char* name, const V& v, const char* tail) {
  printf("\"%s\": [", name);
  size_t j = 0; for (const auto& x : v) printf("%s%d", j++ ? "," : "", (int) x);
  printf("]%s", tail);
}
inline void print_bits_list(const char* name, const float* p, size_t n, const char* tail) {
  printf("\"%s\": [", name);
  for (size_t j = 0; j < n; ++j) printf("%s%u", j ? "," : "", bits(p[j]));
  printf("]%s", tail);
}
inline void print_stats(const lsm2d_iteration_stats& s) {
  printf("\"counts\": [%d,%d,%d], \"chi\": [%u,%u], \"digest\": [%u,%u]", s.n_correspondences, s.n_inliers, s.n_outliers, bits(s.chi_inliers),
         bits(s.chi_outliers), s.pair_digest_lo, s.pair_digest_hi);
}

// ---- two rows (anything with H [9], b [3] and stats) equal byte for byte
template <class R> inline bool same_bytes(const R& a, const R& b) {
  return !memcmp(a.H.data(), b.H.data(), sizeof(float) * 9) && !memcmp(a.b.data(), b.b.data(), sizeof(float) * 3) &&
         !memcmp(&a.stats, &b.stats, sizeof(lsm2d_iteration_stats));
}

// ---- the acceptance test and the total order of the select calls on the host, in fp32 as the kernels evaluate them: more inliers first, then the smaller
// chi^2 sum (its bit pattern orders like the value: it is never negative)
inline bool accept(const lsm2d_iteration_stats& s, const lsm2d_select_params& p) {
  const float n_in = (float) s.n_inliers, n_c = (float) (s.n_correspondences > 1 ? s.n_correspondences : 1);
  return s.n_inliers >= p.min_inliers && s.chi_inliers / (n_in > 1.f ? n_in : 1.f) <= p.max_chi_per_inlier && n_in / n_c >= p.min_inlier_ratio;
}
inline uint64_t key_of(const lsm2d_iteration_stats& s) { return ((uint64_t) (uint32_t) (0x7fffffff - s.n_inliers) << 32) | bits(s.chi_inliers); }
