// lsm2d_voxelize against the route a caller had before it -- lsm2d_cloudset_download per cloud, the same voxelisation on the host (std::sort on (key,
// index), the sums in that order: tests/cpp/voxelize_ref.cpp, linked in), and the result sent up again -- through the bare C ABI, alternating call by call:
//   voxelize_bench points.bin offsets.bin poses.bin|- mode res_bits nres_bits steps warmup
// mode "into_one": every input into group 0 (a map made smaller; with poses: K local maps assembled), the result in a reserved single cloud; the host route
//                  ends in lsm2d_cloudset_upload and a wait for it.
// mode "fleet":    the inputs are first put into a reserved-many set (untimed, before every call of either route); the device route decimates that set IN
//                  PLACE, group k = cloud k; the host route downloads every cloud, voxelises it and makes a new set of the results (lsm2d_cloudset_upload
//                  refuses a set of many clouds: lsm2d_cloudset_create is what a caller has).
// Wall clock round calls that end in their wait, kernel timing off; medians over `steps` after `warmup`.  Before any time is reported the two routes' outputs
// are compared byte for byte.  Prints one JSON line.
#include "driver_common.h"

extern "C" int voxref_voxelize(const float* points, const int32_t* offsets, int n_inputs, const float* pose, const int32_t* group, int n_groups, float resolution,
                               float normal_resolution, float* out, int32_t* counts, int32_t* dropped);

int main(int argc, char** argv) {
  if (argc < 9) { fprintf(stderr, "usage: %s points.bin offsets.bin poses.bin|- into_one|fleet res_bits nres_bits steps warmup\n", argv[0]); return 2; }
  const std::vector<float> pts = read_all<float>(argv[1]);
  const std::vector<int32_t> offs = read_all<int32_t>(argv[2]);
  const std::vector<float> poses = read_all_or_empty<float>(argv[3]);
  const bool fleet = !strcmp(argv[4], "fleet");
  const lsm2d_voxelize_params P{from_bits_arg(argv[5]), from_bits_arg(argv[6])};
  const int steps = atoi(argv[7]), warmup = atoi(argv[8]);
  const int32_t K = (int32_t) offs.size() - 1; const int64_t N = offs[(size_t) K];
  int64_t largest = 1; for (int32_t k = 0; k < K; ++k) largest = std::max<int64_t>(largest, offs[(size_t) k + 1] - offs[(size_t) k]);
  lsm2d_context* ctx = nullptr; must(lsm2d_create(0, nullptr, &ctx), "lsm2d_create", ctx);
  lsm2d_cloudset* src = nullptr; must(lsm2d_cloudset_create(ctx, pts.data(), K > 1 ? offs.data() : nullptr, K, N, &src), "lsm2d_cloudset_create", ctx);
  const int32_t G = fleet ? K : 1;
  std::vector<int32_t> each((size_t) K); for (int32_t k = 0; k < K; ++k) each[(size_t) k] = k;
  std::vector<int32_t> counts((size_t) G), dropped((size_t) G), h_counts((size_t) G), h_dropped((size_t) G), fill_counts((size_t) G);
  std::vector<float> down((size_t) 4 * (size_t) N), h_out((size_t) 4 * (size_t) N), check_a((size_t) 4 * (size_t) N), check_b((size_t) 4 * (size_t) N);
  std::vector<int32_t> h_offs((size_t) K + 1, 0);
  lsm2d_cloudset *dst = nullptr, *dst_host = nullptr, *many = nullptr, *made = nullptr;
  const lsm2d_voxelize_params fill{2.0e-3f, 1.0f};      // the fleet's maps as they go in: a voxelisation so fine that little merges (2 mm cells reach +-65 m)
  if (fleet) must(lsm2d_cloudset_create_reserved_many(ctx, K, largest, &many), "lsm2d_cloudset_create_reserved_many", ctx);
  else { must(lsm2d_cloudset_create_reserved(ctx, N, &dst), "lsm2d_cloudset_create_reserved", ctx); must(lsm2d_cloudset_create_reserved(ctx, N, &dst_host), "lsm2d_cloudset_create_reserved", ctx); }
  auto refill = [&]() { if (fleet) must(lsm2d_voxelize(ctx, &fill, src, K, nullptr, nullptr, each.data(), K, many, nullptr, fill_counts.data(), nullptr), "lsm2d_voxelize (fill)", ctx); };
  auto device_route = [&]() {
    if (fleet) must(lsm2d_voxelize(ctx, &P, many, K, nullptr, nullptr, each.data(), K, many, nullptr, counts.data(), dropped.data()), "lsm2d_voxelize", ctx);
    else must(lsm2d_voxelize(ctx, &P, src, K, nullptr, poses.empty() ? nullptr : poses.data(), nullptr, 1, dst, nullptr, counts.data(), dropped.data()), "lsm2d_voxelize", ctx);
  };
  auto host_route = [&]() {
    const lsm2d_cloudset* from = fleet ? many : src;
    for (int32_t k = 0; k < K; ++k) {
      int64_t n = 0;
      must(lsm2d_cloudset_download(from, k, down.data() + 4 * (size_t) h_offs[(size_t) k], N - h_offs[(size_t) k], &n), "lsm2d_cloudset_download", ctx);
      h_offs[(size_t) k + 1] = h_offs[(size_t) k] + (int32_t) n;
    }
    const int nv = voxref_voxelize(down.data(), h_offs.data(), K, poses.empty() ? nullptr : poses.data(), fleet ? each.data() : nullptr, G, P.resolution, P.normal_resolution,
                                   h_out.data(), h_counts.data(), h_dropped.data());
    if (fleet) {
      std::vector<int32_t> o((size_t) G + 1, 0); for (int32_t g = 0; g < G; ++g) o[(size_t) g + 1] = o[(size_t) g] + h_counts[(size_t) g];
      if (made) { lsm2d_cloudset_destroy(made); made = nullptr; }
      must(lsm2d_cloudset_create(ctx, h_out.data(), o.data(), G, nv, &made), "lsm2d_cloudset_create", ctx);
    } else {
      must(lsm2d_cloudset_upload(dst_host, h_out.data(), nv), "lsm2d_cloudset_upload", ctx);
      must(lsm2d_synchronize(ctx), "lsm2d_synchronize", ctx);
    }
  };
  // ---- parity first (the device route last: in fleet mode its result lies in the set the refill writes)
  refill(); host_route(); refill(); device_route();
  int equal = counts == h_counts && dropped == h_dropped;
  int64_t n_out = 0;
  for (int32_t g = 0; g < G && equal; ++g) {
    int64_t na = 0, nb = 0;
    must(lsm2d_cloudset_download(fleet ? many : dst, g, check_a.data(), N, &na), "lsm2d_cloudset_download", ctx);
    must(lsm2d_cloudset_download(fleet ? made : dst_host, g, check_b.data(), N, &nb), "lsm2d_cloudset_download", ctx);
    equal = na == nb && na == counts[(size_t) g] && !memcmp(check_a.data(), check_b.data(), sizeof(float) * 4 * (size_t) na);
    n_out += na;
  }
  // ---- times, the routes alternating call by call
  std::vector<double> td, th;
  for (int i = 0; i < warmup + steps; ++i) {
    refill();
    double t0 = now_ms(); device_route(); double t1 = now_ms();
    refill();
    double t2 = now_ms(); host_route(); double t3 = now_ms();
    if (i >= warmup) { td.push_back(t1 - t0); th.push_back(t3 - t2); }
  }
  double d[3], h[3]; summary(td, d, true); summary(th, h, true);      // the upper middle element, as ever
  float kernel_ms = 0.0f;
  must(lsm2d_set_option(ctx, "kernel_timing", 1), "lsm2d_set_option", ctx);
  refill(); device_route();
  must(lsm2d_last_kernel_ms(ctx, &kernel_ms), "lsm2d_last_kernel_ms", ctx);
  printf("{\"mode\": \"%s\", \"inputs\": %d, \"points\": %lld, \"voxels\": %lld, \"outputs_equal\": %d, \"device_ms\": [%.4f, %.4f, %.4f], \"host_route_ms\": [%.4f, %.4f, %.4f], "
         "\"device_kernel_ms\": %.4f}\n", argv[4], K, (long long) N, (long long) n_out, equal, d[0], d[1], d[2], h[0], h[1], h[2], kernel_ms);
  for (lsm2d_cloudset* s : {src, dst, dst_host, many, made}) if (s) lsm2d_cloudset_destroy(s);
  lsm2d_destroy(ctx);
  return equal ? 0 : 3;
}
