// mirror_trace_driver.cpp -- one script over every public function and class method of host/lsm2d.hpp, linked against tests/cpp/lsm2d_standin.cpp instead of
// the library: the stand-in writes the record of the C calls to stdout, this driver adds what came back to it ("= ...") and, for every refusal it walks,
// "throws: <what()>".  Every scene makes its own Context and is followed by the stand-in's leak check; the exit status is 4 when a handle leaked, 3 when the
// stand-in saw a handle after its destroy, else 0.  Nothing computes; the shapes are tiny.  tests/test_cpp_mirror_calls_cpu.py compares the record with
// tests/golden/cpp_mirror_call_trace.json.
#include <lsm2d.hpp>

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

extern "C" {
void standin_fail_at(const char* symbol, int kth);
void standin_select(int32_t n, const int32_t* index);
void standin_note(const char* text);
int standin_leak_check(const char* where);
}

using namespace lsm2d_host;

static int g_leaks = 0;

static void note(const std::string& s) { standin_note(s.c_str()); }
static void select(std::vector<int32_t> idx) { standin_select((int32_t) idx.size(), idx.data()); }
// a scene: its objects die before the leak check; what it throws is part of the record
static void scene(const std::string& name, const std::function<void()>& body) {
  note("# " + name);
  try { body(); }
  catch (const std::runtime_error& e) { note(std::string("throws: ") + e.what()); }
  catch (const std::out_of_range&) { note("throws std::out_of_range"); }
  standin_fail_at("", 0);
  g_leaks += standin_leak_check(name.c_str());
}
static void failing(const std::string& name, const char* symbol, int kth, const std::function<void()>& body) {
  scene(name, [&] { standin_fail_at(symbol, kth); body(); note("no throw"); });
}

template <class T> static std::string list(const T* v, size_t n) {
  std::string s = "[";
  for (size_t i = 0; i < n; ++i) s += (i ? " " : "") + std::to_string(v[i]);
  return s + "]";
}
static std::string str(const lsm2d_iteration_stats& st) {
  return "{" + std::to_string(st.n_correspondences) + " " + std::to_string(st.n_inliers) + " " + std::to_string(st.n_outliers) + " " + std::to_string(st.chi_inliers) + " " +
         std::to_string(st.chi_outliers) + " " + std::to_string(st.pair_digest_lo) + " " + std::to_string(st.pair_digest_hi) + "}";
}
static std::string str(const Linearization& r) { return "H" + list(r.H.data(), 9) + " b" + list(r.b.data(), 3) + " " + str(r.stats); }
static void show(const std::vector<Linearization>& rows) { note("= " + std::to_string(rows.size()) + " rows"); for (const auto& r : rows) note("=   " + str(r)); }
static void show(const std::vector<AlignerScore>& rows) {
  note("= " + std::to_string(rows.size()) + " rows");
  for (const auto& r : rows) note("=   " + str(r.row) + " active " + std::to_string(r.active));
}
static void show(const std::vector<CorrespondenceVector>& pairs) {
  for (const auto& v : pairs) { std::string s = "= pairs"; for (const auto& c : v) s += " (" + std::to_string(c.fixed_idx) + "," + std::to_string(c.moving_idx) + ")"; note(s); }
}
template <class R> static void showAligned(const R& r) {      // the tail both relocalize overloads share
  note("= pose " + std::to_string(r.pose.size()) + " information " + std::to_string(r.information.size()) + " status " + list(r.status.data(), r.status.size()) +
       " iterations " + list(r.iterations.data(), r.iterations.size()) + " accepted " + list(r.accepted.data(), r.accepted.size()));
  for (size_t j = 0; j < r.pose.size(); ++j) note("=   pose" + list(r.pose[j].data(), 3) + " information" + list(r.information[j].data(), 9) + " " + str(r.last_stats[j]));
}

static PointNormal2fVectorCloud cloud(size_t n, float shift) {
  PointNormal2fVectorCloud c(n);
  for (size_t i = 0; i < n; ++i) c[i] = PointNormal2f{shift + (float) i, shift - (float) i, 0.6f, 0.8f};
  return c;
}
static const std::vector<Vector3f> POSES = {Vector3f{{0.1f, 0.2f, 0.3f}}, Vector3f{{-0.4f, 0.5f, -0.6f}}, Vector3f{{0.7f, -0.8f, 0.9f}}};
static std::vector<lsm2d_prior> priors(size_t n) {
  std::vector<lsm2d_prior> p(n);
  for (size_t i = 0; i < n; ++i) { for (int k = 0; k < 3; ++k) p[i].z[k] = 0.1f * (float) (i + 1) + (float) k; for (int k = 0; k < 9; ++k) p[i].omega[k] = (float) (10 * i + (size_t) k); }
  return p;
}
static lsm2d_slice_params slice(float sensor_x) {
  PointNormal2fProjectorPolar pr; pr.param_canvas_cols = 8;
  lsm2d_slice_params sp = LoopClosureSweep::projectiveSlice(pr, 0.5f, 0.8f, 0.05f, 2);
  sp.sensor_in_robot[0] = sensor_x;
  return sp;
}
static const lsm2d_aligner_params ALIGNER{3, 2, 0.5f, 1e-3f, 1, 0};
static const lsm2d_select_params SELECT{2, 0.5f, 0.25f};
static const std::vector<int32_t> NONE;

static void contextAndSets() {
  Context ctx(1);
  ctx.setKernelTiming(true); ctx.setOption("align_path", 2);
  note("= option " + std::to_string(ctx.getOption("last_align_path")) + " ms " + std::to_string(ctx.lastKernelMs()));
  CloudSet one(ctx, cloud(5, 1.f)), none(ctx, PointNormal2fVectorCloud{});
  CloudSet many(ctx, std::vector<PointNormal2fVectorCloud>{cloud(3, 0.f), cloud(4, 2.f), cloud(6, 5.f)}), empty(ctx, std::vector<PointNormal2fVectorCloud>{});
  note("= numClouds " + std::to_string(one.numClouds()) + " " + std::to_string(many.numClouds()) + " " + std::to_string(empty.numClouds()) + " " + std::to_string(none.get() != nullptr));
  ReservedCloud r(ctx, 64);
  r.upload(cloud(4, 3.f)); r.upload({});
  r.upload(cloud(6, 3.f));
  note("= size " + std::to_string(r.size()) + " downloaded " + std::to_string(r.download().size()) + " " + std::to_string(r.get() != nullptr));
}

static void freeFunctions() {
  Context ctx;
  const CloudSet one(ctx, cloud(5, 1.f)), many(ctx, std::vector<PointNormal2fVectorCloud>{cloud(3, 0.f), cloud(4, 2.f), cloud(6, 5.f)});
  const lsm2d_slice_params sp = slice(0.f);
  lsm2d_slice_params nn = sp; nn.finder = LSM2D_FINDER_NN;
  const std::vector<int32_t> fi{2, 0, 1}, mi{1, 1, 0};
  const std::vector<Vector3f> no_poses;
  show(findCorrespondencesBatch(ctx, sp, one, many, POSES, NONE, NONE));
  show(findCorrespondencesBatch(ctx, nn, many, many, POSES, fi, mi));
  show(findCorrespondencesBatch(ctx, nn, one, one, no_poses, NONE, NONE));
  const CorrespondenceVector pairs{{0, 1}, {1, 2}, {2, 0}};
  note("= " + str(linearize(ctx, sp, one, many, pairs, POSES[0])));
  note("= " + str(linearize(ctx, sp, many, one, {}, POSES[1], 2, 0)));
  const std::vector<CorrespondenceVector> rows{pairs, {}, {{3, 3}}};
  show(linearizeBatch(ctx, sp, one, many, rows, POSES));
  show(linearizeBatch(ctx, sp, many, many, rows, POSES, fi, mi));
  show(linearizeBatch(ctx, sp, one, one, {}, no_poses));
  show(scoreBatch(ctx, sp, one, many, POSES));
  show(scoreBatch(ctx, sp, many, many, POSES, fi, mi));
  show(scoreBatch(ctx, sp, one, one, no_poses));
  for (int form = 0; form < 3; ++form) {
    if (form < 2) select({2, 0});
    const Selection s = form == 1 ? scoreSelect(ctx, sp, many, many, POSES, SELECT, 3, fi, mi) : scoreSelect(ctx, sp, one, many, POSES, SELECT, form ? 0 : 2);
    note("= index " + list(s.index.data(), s.index.size()) + " n_accepted " + std::to_string(s.n_accepted)); show(s.rows);
  }
  const lsm2d_iteration_stats cases[] = {{0, 0, 0, 0.f, 0.f, 0, 0}, {1, 1, 0, 0.1f, 0.f, 0, 0}, {10, 8, 2, 0.8f, 0.f, 0, 0}, {10, 7, 3, 7.f, 0.f, 0, 0}, {10, 2, 8, 0.f, 0.f, 0, 0}};
  std::string verdicts = "= selectAccept";
  for (const auto& st : cases) verdicts += selectAccept(st, SELECT) ? " 1" : " 0";
  note(verdicts);
}

static void relocalizeOneSlice() {
  Context ctx;
  const CloudSet one(ctx, cloud(5, 1.f)), many(ctx, std::vector<PointNormal2fVectorCloud>{cloud(3, 0.f), cloud(4, 2.f), cloud(6, 5.f)});
  const lsm2d_slice_params sp = slice(0.f);
  const std::vector<int32_t> fi{2, 0, 1}, mi{1, 1, 0};
  for (int form = 0; form < 4; ++form) {          // one-cloud fixed set; both sets indexed; every set one cloud; nothing selected
    if (form < 3) select({2, 0});
    const Relocalization r = form == 1 ? relocalize(ctx, ALIGNER, sp, many, many, POSES, SELECT, 2, fi, mi)
                             : form == 2 ? relocalize(ctx, ALIGNER, sp, one, one, POSES, SELECT, 2) : relocalize(ctx, ALIGNER, sp, one, many, POSES, SELECT, 2);
    note("= index " + list(r.selection.index.data(), r.selection.index.size()) + " n_accepted " + std::to_string(r.selection.n_accepted)); show(r.selection.rows);
    showAligned(r);
  }
}

static void alignerFunctions() {
  Context ctx;
  const CloudSet one(ctx, cloud(5, 1.f)), many(ctx, std::vector<PointNormal2fVectorCloud>{cloud(3, 0.f), cloud(4, 2.f), cloud(6, 5.f)});
  const std::vector<lsm2d_slice_params> slices{slice(0.2f), slice(-0.3f)}, single{slice(0.f)};
  const std::vector<const CloudSet*> fixed{&many, &one}, moving{&one, &many}, f1{&many}, m1{&one}, all_one{&one, &one};
  const std::vector<int32_t> fi{2, 0, 1, 0, 0, 0}, mi{0, 0, 0, 1, 1, 2};
  const std::vector<lsm2d_prior> pr = priors(3);
  show(scoreAligner(ctx, slices, fixed, moving, POSES));
  show(scoreAligner(ctx, slices, fixed, moving, POSES, pr, fi, mi));
  show(scoreAligner(ctx, single, f1, m1, {}));
  for (int form = 0; form < 3; ++form) {
    if (form < 2) select({1, 2});
    const AlignerSelection s = form == 1 ? scoreAlignerSelect(ctx, slices, fixed, moving, POSES, SELECT, 3, pr, fi, mi) : scoreAlignerSelect(ctx, single, f1, m1, POSES, SELECT, form ? 0 : 1);
    note("= index " + list(s.index.data(), s.index.size()) + " n_accepted " + std::to_string(s.n_accepted)); show(s.rows);
  }
  for (int form = 0; form < 3; ++form) {
    if (form < 2) select({1, 2});
    const AlignSelection s = form == 1 ? alignSelect(ctx, ALIGNER, slices, fixed, moving, POSES, SELECT, 3, pr, fi, mi) : alignSelect(ctx, ALIGNER, single, f1, m1, POSES, SELECT, form ? 0 : 1);
    note("= index " + list(s.index.data(), s.index.size()) + " n_accepted " + std::to_string(s.n_accepted) + " n_success " + std::to_string(s.n_success) + " iterations " +
         list(s.iterations.data(), s.iterations.size()));
    for (size_t j = 0; j < s.pose.size(); ++j) note("=   pose" + list(s.pose[j].data(), 3) + " information" + list(s.information[j].data(), 9) + " " + str(s.last_stats[j]));
  }
  for (int form = 0; form < 5; ++form) {          // no index vectors, no priors; both; one-cloud sets only; one slice; nothing selected
    if (form < 4) select({2, 1});
    const AlignerRelocalization r = form == 1   ? relocalize(ctx, ALIGNER, slices, fixed, moving, POSES, SELECT, 2, pr, fi, mi)
                                    : form == 2 ? relocalize(ctx, ALIGNER, slices, all_one, all_one, POSES, SELECT, 2, pr)
                                    : form == 3 ? relocalize(ctx, ALIGNER, single, f1, m1, POSES, SELECT, 2)
                                                : relocalize(ctx, ALIGNER, slices, fixed, moving, POSES, SELECT, 2);
    note("= index " + list(r.selection.index.data(), r.selection.index.size()) + " n_accepted " + std::to_string(r.selection.n_accepted)); show(r.selection.rows);
    showAligned(r);
  }
}

static void finders() {
  Context ctx;
  const PointNormal2fVectorCloud a = cloud(5, 1.f), b = cloud(4, 2.f);
  const CloudSet one(ctx, a), many(ctx, std::vector<PointNormal2fVectorCloud>{cloud(3, 0.f), cloud(4, 2.f)});
  const std::vector<int32_t> fi{1, 0, 1}, mi{0, 0, 1};
  CorrespondenceVector out;
  auto shown = [&](const char* what) { std::string s = std::string("= ") + what; for (const auto& c : out) s += " (" + std::to_string(c.fixed_idx) + "," + std::to_string(c.moving_idx) + ")"; note(s); };
  CorrespondenceFinderProjective2f proj(ctx);
  proj.param_projector->param_canvas_cols = 8; proj.param_point_distance = 0.4f; proj.param_normal_cos = 0.7f;
  proj.setFixed(&a); proj.setMoving(&b); proj.setLocalMapInSensor(POSES[0]); proj.setCorrespondences(&out);
  proj.compute(); shown("projective");
  proj.setFixed(&b); proj.compute(); shown("projective");
  show(proj.computeBatch(one, many, POSES)); show(proj.computeBatch(many, many, POSES, fi, mi));
  CorrespondenceFinderKDTree2D kd(ctx), exact(ctx, "exact");
  kd.param_max_leaf_range = 0.05f; kd.param_min_leaf_points = 3;
  CorrespondenceFinderNN2D dm(ctx);
  dm.param_resolution = 0.1f;
  for (CorrespondenceFinderPointQuery* f : {(CorrespondenceFinderPointQuery*) &kd, (CorrespondenceFinderPointQuery*) &exact, (CorrespondenceFinderPointQuery*) &dm}) {
    f->setFixed(&a); f->setMoving(&b); f->setLocalMapInSensor(POSES[1]); f->setCorrespondences(&out);
    f->compute(); shown("point query");
    show(f->computeBatch(one, many, POSES)); show(f->computeBatch(many, many, POSES, fi, mi));
  }
  kd.setSearch("exact"); kd.setMoving(&a); kd.compute(); shown("point query");
  kd.setSearch("kdtree"); kd.compute(); shown("point query");
}

static void mapping() {
  Context ctx;
  ReservedCloud scene(ctx, 64), clipped(ctx, 8), meas(ctx, 8);
  const PointNormal2fVectorCloud m = cloud(4, 2.f);
  for (int asynchronous = 0; asynchronous < 2; ++asynchronous) {
    SceneClipperProjective2D clip(ctx);
    clip.param_projector->param_canvas_cols = 8; clip.asynchronous = asynchronous != 0;
    clip.setFullScene(&scene); clip.setClippedSceneInRobot(&clipped); clip.setRobotInLocalMap(POSES[0]); clip.setSensorInRobot(POSES[1]);
    note("= clipped " + std::to_string(clip.compute()));
    clip.param_voxelize_resolution = 0.f;
    note("= clipped " + std::to_string(clip.compute()));
    MergerProjective2D merge(ctx);
    merge.param_projector->param_canvas_cols = 8; merge.param_merge_threshold = 0.25f; merge.asynchronous = asynchronous != 0;
    merge.setScene(&scene); merge.setMeasurementInScene(POSES[2]);
    merge.setMeasurement(&m);
    note("= merged " + std::to_string(merge.compute()) + " counts " + list(merge.counts.data(), 3));
    merge.setMeasurement(&meas);
    note("= merged " + std::to_string(merge.compute()) + " counts " + list(merge.counts.data(), 3));
    note("= merged " + std::to_string(merge.computeAll({&meas, &clipped}, {POSES[0], POSES[1]})));
  }
}

static std::shared_ptr<AlignerSliceProcessorLaser2D> processor(Context& ctx, const char* fixed_name, bool robust, float sensor_x) {
  auto s = std::make_shared<AlignerSliceProcessorLaser2D>();
  s->param_fixed_slice_name = fixed_name; s->param_min_num_correspondences = 2; s->sensor_in_robot = Vector3f{{sensor_x, 0.f, 0.f}};
  s->param_finder = std::make_shared<CorrespondenceFinderProjective2f>(ctx);
  s->param_finder->param_projector->param_canvas_cols = 8;
  if (robust) { s->param_robustifier = std::make_shared<RobustifierCauchy>(); s->param_robustifier->param_chi_threshold = 0.02f; }
  return s;
}
static void multiAligner() {
  Context ctx;
  const PointNormal2fVectorCloud a = cloud(5, 1.f), b = cloud(4, 2.f), c = cloud(6, 0.f);
  const MultiAligner2D::PropertyContainer fixed{{"points", &a}, {"rear", &b}}, moving{{"points", &c}};
  MultiAligner2D al(ctx);
  al.param_max_iterations = 3; al.param_min_num_inliers = 2; al.param_damping = 0.5f; al.param_termination_chi_epsilon = 1e-3f; al.param_enable_inlier_only_runs = true;
  al.param_slice_processors = {processor(ctx, "points", true, 0.2f), processor(ctx, "rear", false, -0.3f)};
  al.setFixed(&fixed); al.setMoving(&moving);
  for (int form = 0; form < 4; ++form) {          // store_correspondences off / on, without and with a prior
    al.store_correspondences = (form & 1) != 0;
    if (form == 2) al.setPrior(Vector3f{{0.1f, 0.f, -0.1f}}, std::array<float, 9>{{7, 0, 0, 0, 7, 0, 0, 0, 7}});
    al.setMovingInFixed(POSES[(size_t) form % 3]);
    al.compute();
    note("= status " + std::to_string(al.status()) + " pose" + list(al.movingInFixed().data(), 3) + " information" + list(al.informationMatrix().data(), 9) + " stats " +
         std::to_string(al.iterationStats().size()) + " pairs " + std::to_string(al.correspondences(0).size()) + " " + std::to_string(al.correspondences(1).size()));
    for (const auto& st : al.iterationStats()) note("=   " + str(st));
  }
}

static void stream() {
  Context ctx;
  const CloudSet map(ctx, cloud(6, 0.f));
  const lsm2d_preprocessor pre{4, -1.5f, 1.5f, 0.3f, 20.f, 0.3f, 3, 0.02f};
  LaserMessageBatchStream s(ctx, pre, map, slice(0.f), ALIGNER, 2);
  auto results = [&](bool ready) {
    note("= " + std::to_string(ready) + " retired " + std::to_string(s.retired()));
    if (ready) note("=   status " + list(s.status.data(), s.status.size()) + " iterations " + list(s.iterations.data(), s.iterations.size()) + " information" + list(s.information[1].data(), 9));
  };
  results(false);
  for (int k = 0; k < 5; ++k) {
    std::vector<float> ranges(8); for (size_t i = 0; i < 8; ++i) ranges[i] = 1.f + (float) k + 0.1f * (float) i;
    const Vector3f start[2] = {POSES[(size_t) k % 3], POSES[(size_t) (k + 1) % 3]};
    results(s.push(ranges.data(), start));
  }
  bool more = true;
  while (more) { more = s.flush(); results(more); }
  results(s.flush());
}
static void streamLeftToItsDestructor() {
  Context ctx;
  const CloudSet map(ctx, cloud(6, 0.f));
  const lsm2d_preprocessor pre{4, -1.5f, 1.5f, 0.3f, 20.f, 0.3f, 3, 0.02f};
  LaserMessageBatchStream s(ctx, pre, map, slice(0.f), ALIGNER, 1);
  const std::vector<float> ranges{1.f, 2.f, 3.f, 4.f};
  for (int k = 0; k < 2; ++k) s.push(ranges.data(), &POSES[0]);
}

static TrackerBatch::Params trackerParams(float voxelize) {
  TrackerBatch::Params p;
  p.projector.canvas_cols = 8; p.preprocessor.n_beams = 4; p.slices = {{slice(0.2f), slice(-0.3f)}}; p.aligner = ALIGNER; p.map_capacity = 32; p.clip_voxelize_resolution = voxelize;
  return p;
}
static const float FRONT[12] = {1.f, 1.1f, 1.2f, 1.3f, 2.f, 2.1f, 2.2f, 2.3f, 3.f, 3.1f, 3.2f, 3.3f}, REAR[12] = {4.f, 4.1f, 4.2f, 4.3f, 5.f, 5.1f, 5.2f, 5.3f, 6.f, 6.1f, 6.2f, 6.3f};
static const double START[6] = {0.5, -0.5, 0.25, 1.0, 2.0, -3.0}, ODOMETRY[9] = {0.1, 0.0, 0.01, 0.0, 0.1, -0.02, 0.05, 0.05, 3.1};
static const int32_t BOTH[2] = {2, 0};
static void trackers(float voxelize) {
  Context ctx;
  TrackerBatch tb(ctx, 3, trackerParams(voxelize));
  tb.reset(2, BOTH, FRONT, REAR, START);
  for (int k = 0; k < 2; ++k) {                   // the first step makes the scan sets, the second refills them
    tb.step(FRONT, REAR, ODOMETRY);
    note("= size " + std::to_string(tb.size()) + " pose" + list(tb.movingInFixed().data(), 9) + " status " + list(tb.status().data(), 3) + " information " +
         std::to_string(tb.informationMatrix().size()) + " estimate" + list(tb.robotInLocalMap().data(), 9) + " " + std::to_string(tb.localMaps() != tb.clippedScenes()));
  }
}

static void sweep() {
  LoopClosureSweep sw({0, 1});
  note("= devices " + std::to_string(sw.numDevices()));
  sw.param_max_iterations = 5; sw.param_slice = slice(0.f);
  sw.param_relocalize_min_inliers = 6; sw.param_relocalize_max_chi_inliers = 0.5f; sw.param_relocalize_min_inliers_ratio = 0.25f;
  sw.setMap(cloud(6, 0.f)); sw.setMap({});
  sw.setScans({cloud(3, 0.f), cloud(4, 2.f)});
  const std::vector<float> packed{1, 2, 0, 1, 3, 4, 1, 0, 5, 6, 0, 1}; const std::vector<int32_t> offs{0, 1, 3};
  sw.setScansPacked(packed.data(), offs.data(), 2);
  sw.compute({1, 0, 1}, POSES);
  std::string verdicts = "= accept";
  for (size_t i = 0; i < 3; ++i) verdicts += sw.accept(i) ? " 1" : " 0";
  note(verdicts + " status " + list(sw.status.data(), 3) + " iterations " + list(sw.iterations.data(), 3));
  sw.last_stats[0] = {0, 0, 0, 0.f, 0.f, 0, 0}; sw.last_stats[1] = {10, 8, 2, 0.8f, 0.f, 0, 0}; sw.last_stats[2] = {10, 7, 3, 7.f, 0.f, 0, 0}; sw.status[1] = 1;
  sw.param_relocalize_min_inliers = 0;
  note(std::string("= accept ") + (sw.accept(0) ? "1" : "0") + (sw.accept(1) ? " 1" : " 0") + (sw.accept(2) ? " 1" : " 0"));
  sw.compute({}, {});
  for (int32_t k : {2, 0}) {
    select({2, 0});
    sw.computeSelect({1, 0, 1}, POSES, k);
    note("= selected " + list(sw.selected.data(), sw.selected.size()) + " n_accepted " + std::to_string(sw.n_accepted) + " n_success " + std::to_string(sw.n_success) + " pose " +
         std::to_string(sw.pose.size()) + " information " + std::to_string(sw.information.size()) + " status " + std::to_string(sw.status.size()) + " iterations " +
         list(sw.iterations.data(), sw.iterations.size()) + " last_stats " + std::to_string(sw.last_stats.size()));
  }
}

// every throw a caller can reach without a device, and one failing C call per class
static void refusals() {
  const std::vector<int32_t> two{0, 1}, fi{2, 0, 1}, six{0, 0, 0, 0, 0, 0};
  const lsm2d_slice_params sp = slice(0.f);
  const PointNormal2fVectorCloud a = cloud(5, 1.f), b = cloud(4, 2.f);
  struct Sets { Context ctx; CloudSet one, many; Sets() : one(ctx, cloud(5, 1.f)), many(ctx, std::vector<PointNormal2fVectorCloud>{cloud(3, 0.f), cloud(4, 2.f), cloud(6, 5.f)}) {} };

  failing("Context: create fails", "lsm2d_create", 1, [] { Context ctx; });
  failing("Context: set_option fails", "lsm2d_set_option", 1, [] { Context ctx; ctx.setKernelTiming(false); });
  failing("Context: setOption fails", "lsm2d_set_option", 1, [] { Context ctx; ctx.setOption("align_path", 1); });
  failing("Context: get_option fails", "lsm2d_get_option", 1, [] { Context ctx; ctx.getOption("align_path"); });
  failing("Context: last_kernel_ms fails", "lsm2d_last_kernel_ms", 1, [] { Context ctx; ctx.lastKernelMs(); });
  failing("CloudSet: create fails", "lsm2d_cloudset_create", 1, [&] { Context ctx; CloudSet s(ctx, a); });
  failing("CloudSet: ragged create fails", "lsm2d_cloudset_create", 1, [&] { Context ctx; CloudSet s(ctx, std::vector<PointNormal2fVectorCloud>{a, b}); });
  failing("ReservedCloud: create fails", "lsm2d_cloudset_create_reserved", 1, [] { Context ctx; ReservedCloud r(ctx, 8); });
  failing("ReservedCloud: upload fails", "lsm2d_cloudset_upload", 1, [&] { Context ctx; ReservedCloud r(ctx, 8); r.upload(a); });
  failing("ReservedCloud: download fails", "lsm2d_cloudset_download", 1, [&] { Context ctx; ReservedCloud r(ctx, 8); r.upload(a); r.download(); });

  for (int which = 0; which < 2; ++which) {
    const std::vector<int32_t>& f = which ? NONE : two; const std::vector<int32_t>& m = which ? two : NONE;
    scene("findCorrespondencesBatch: index vector", [&] { Sets s; findCorrespondencesBatch(s.ctx, sp, s.many, s.many, POSES, f, m); });
    scene("linearizeBatch: index vector", [&] { Sets s; linearizeBatch(s.ctx, sp, s.many, s.many, {{}, {}, {}}, POSES, f, m); });
    scene("scoreBatch: index vector", [&] { Sets s; scoreBatch(s.ctx, sp, s.many, s.many, POSES, f, m); });
    scene("scoreSelect: index vector", [&] { Sets s; scoreSelect(s.ctx, sp, s.many, s.many, POSES, SELECT, 2, f, m); });
    scene("relocalize: index vector", [&] { Sets s; relocalize(s.ctx, ALIGNER, sp, s.many, s.many, POSES, SELECT, 2, f, m); });
    scene("alignSelect: index vector", [&] { Sets s; alignSelect(s.ctx, ALIGNER, {sp, sp}, {&s.many, &s.one}, {&s.one, &s.many}, POSES, SELECT, 2, {}, which ? NONE : fi, which ? fi : NONE); });
    scene("scoreAligner: index vector", [&] { Sets s; scoreAligner(s.ctx, {sp, sp}, {&s.many, &s.one}, {&s.one, &s.many}, POSES, {}, which ? NONE : fi, which ? fi : NONE); });
    scene("scoreAlignerSelect: index vector", [&] { Sets s; scoreAlignerSelect(s.ctx, {sp, sp}, {&s.many, &s.one}, {&s.one, &s.many}, POSES, SELECT, 2, {}, which ? NONE : fi, which ? fi : NONE); });
    scene("relocalize (aligner): index vector", [&] { Sets s; relocalize(s.ctx, ALIGNER, {sp, sp}, {&s.many, &s.one}, {&s.one, &s.many}, POSES, SELECT, 2, {}, which ? NONE : fi, which ? fi : NONE); });
    const std::vector<const CloudSet*> none;
    scene("alignSelect: sets per slice", [&] { Sets s; std::vector<const CloudSet*> ok{&s.one}; alignSelect(s.ctx, ALIGNER, {sp}, which ? ok : none, which ? none : ok, POSES, SELECT, 2); });
    scene("scoreAligner: sets per slice", [&] { Sets s; std::vector<const CloudSet*> ok{&s.one}; scoreAligner(s.ctx, {sp}, which ? ok : none, which ? none : ok, POSES); });
    scene("scoreAlignerSelect: sets per slice", [&] { Sets s; std::vector<const CloudSet*> ok{&s.one}; scoreAlignerSelect(s.ctx, {sp}, which ? ok : none, which ? none : ok, POSES, SELECT, 2); });
    scene("relocalize (aligner): sets per slice", [&] { Sets s; std::vector<const CloudSet*> ok{&s.one}; relocalize(s.ctx, ALIGNER, {sp}, which ? ok : none, which ? none : ok, POSES, SELECT, 2); });
  }
  scene("linearizeBatch: one vector per pose", [&] { Sets s; linearizeBatch(s.ctx, sp, s.many, s.many, {{}, {}}, POSES); });
  scene("alignSelect: priors", [&] { Sets s; alignSelect(s.ctx, ALIGNER, {sp}, {&s.many}, {&s.one}, POSES, SELECT, 2, priors(2)); });
  scene("alignSelect: priors beside good index vectors", [&] { Sets s; alignSelect(s.ctx, ALIGNER, {sp, sp}, {&s.many, &s.one}, {&s.one, &s.many}, POSES, SELECT, 2, priors(1), six, six); });
  scene("scoreAligner: priors", [&] { Sets s; scoreAligner(s.ctx, {sp}, {&s.many}, {&s.one}, POSES, priors(2)); });
  scene("scoreAlignerSelect: priors", [&] { Sets s; scoreAlignerSelect(s.ctx, {sp}, {&s.many}, {&s.one}, POSES, SELECT, 2, priors(4)); });
  scene("relocalize (aligner): priors", [&] { Sets s; relocalize(s.ctx, ALIGNER, {sp}, {&s.many}, {&s.one}, POSES, SELECT, 2, priors(2)); });
  lsm2d_slice_params nn = sp; nn.finder = LSM2D_FINDER_NN;
  failing("findCorrespondencesBatch: call fails", "lsm2d_find_correspondences_batch", 1, [&] { Sets s; findCorrespondencesBatch(s.ctx, nn, s.many, s.many, POSES, NONE, NONE); });
  failing("findCorrespondencesBatch: sizes call fails", "lsm2d_cloudset_cloud_sizes", 1, [&] { Sets s; findCorrespondencesBatch(s.ctx, nn, s.many, s.many, POSES, NONE, NONE); });
  failing("linearize: call fails", "lsm2d_linearize", 1, [&] { Sets s; linearize(s.ctx, sp, s.one, s.one, {}, POSES[0]); });
  failing("linearizeBatch: call fails", "lsm2d_linearize_batch", 1, [&] { Sets s; linearizeBatch(s.ctx, sp, s.many, s.many, {{}, {}, {}}, POSES); });
  failing("scoreBatch: call fails", "lsm2d_score_batch", 1, [&] { Sets s; scoreBatch(s.ctx, sp, s.many, s.many, POSES); });
  failing("scoreSelect: call fails", "lsm2d_score_select", 1, [&] { Sets s; scoreSelect(s.ctx, sp, s.many, s.many, POSES, SELECT, 2); });
  failing("relocalize: score call fails", "lsm2d_score_select", 1, [&] { Sets s; relocalize(s.ctx, ALIGNER, sp, s.many, s.many, POSES, SELECT, 2); });
  failing("relocalize: align call fails", "lsm2d_align_batch", 1, [&] { Sets s; select({1}); relocalize(s.ctx, ALIGNER, sp, s.many, s.many, POSES, SELECT, 2); });
  failing("alignSelect: call fails", "lsm2d_align_select", 1, [&] { Sets s; alignSelect(s.ctx, ALIGNER, {sp}, {&s.many}, {&s.one}, POSES, SELECT, 2); });
  failing("scoreAligner: call fails", "lsm2d_score_aligner_batch", 1, [&] { Sets s; scoreAligner(s.ctx, {sp}, {&s.many}, {&s.one}, POSES); });
  failing("scoreAlignerSelect: call fails", "lsm2d_score_aligner_select", 1, [&] { Sets s; scoreAlignerSelect(s.ctx, {sp}, {&s.many}, {&s.one}, POSES, SELECT, 2); });
  failing("relocalize (aligner): score call fails", "lsm2d_score_aligner_select", 1, [&] { Sets s; relocalize(s.ctx, ALIGNER, {sp}, {&s.many}, {&s.one}, POSES, SELECT, 2); });
  failing("relocalize (aligner): align call fails", "lsm2d_align_batch", 1, [&] { Sets s; select({1}); relocalize(s.ctx, ALIGNER, {sp}, {&s.many}, {&s.one}, POSES, SELECT, 2); });

  CorrespondenceVector out;
  scene("projective finder: projector", [&] { Context ctx; CorrespondenceFinderProjective2f f(ctx); f.param_projector.reset(); f.compute(); });
  scene("projective finder: fixed", [&] { Context ctx; CorrespondenceFinderProjective2f f(ctx); f.setFixed(&a); f.setFixed(nullptr); f.setMoving(&b); f.setCorrespondences(&out); f.compute(); });
  scene("projective finder: moving", [&] { Context ctx; CorrespondenceFinderProjective2f f(ctx); f.setFixed(&a); f.setMoving(&b); f.setMoving(nullptr); f.compute(); });
  scene("projective finder: correspondences", [&] { Context ctx; CorrespondenceFinderProjective2f f(ctx); f.setFixed(&a); f.setMoving(&b); f.compute(); });
  scene("projective finder: batch projector", [&] { Sets s; CorrespondenceFinderProjective2f f(s.ctx); f.param_projector.reset(); f.computeBatch(s.one, s.one, POSES); });
  failing("projective finder: call fails", "lsm2d_find_correspondences", 1, [&] { Context ctx; CorrespondenceFinderProjective2f f(ctx); f.setFixed(&a); f.setMoving(&b); f.setCorrespondences(&out); f.compute(); });
  scene("distance-map finder: resolution before anything else", [&] { Context ctx; CorrespondenceFinderNN2D f(ctx); f.param_resolution = 0.f; f.compute(); });
  scene("distance-map finder: batch resolution", [&] { Sets s; CorrespondenceFinderNN2D f(s.ctx); f.param_resolution = -1.f; f.computeBatch(s.one, s.one, POSES); });
  scene("kd-tree finder: resolution is not its concern", [&] { Context ctx; CorrespondenceFinderKDTree2D f(ctx); f.param_resolution = 0.f; f.compute(); });
  scene("point-query finder: fixed", [&] { Context ctx; CorrespondenceFinderNN2D f(ctx); f.setMoving(&b); f.setCorrespondences(&out); f.compute(); });
  scene("point-query finder: moving", [&] { Context ctx; CorrespondenceFinderNN2D f(ctx); f.setFixed(&a); f.setCorrespondences(&out); f.compute(); });
  scene("point-query finder: correspondences", [&] { Context ctx; CorrespondenceFinderNN2D f(ctx); f.setFixed(&a); f.setMoving(&b); f.compute(); });
  scene("kd-tree finder: search", [&] { Context ctx; CorrespondenceFinderKDTree2D f(ctx, "octree"); });
  scene("kd-tree finder: setSearch", [&] { Context ctx; CorrespondenceFinderKDTree2D f(ctx); f.setSearch("grid"); });
  failing("point-query finder: call fails", "lsm2d_find_correspondences", 1, [&] { Context ctx; CorrespondenceFinderKDTree2D f(ctx); f.setFixed(&a); f.setMoving(&b); f.setCorrespondences(&out); f.compute(); });
  failing("point-query finder: upload fails", "lsm2d_cloudset_create", 2, [&] { Context ctx; CorrespondenceFinderKDTree2D f(ctx); f.setFixed(&a); f.setMoving(&b); });

  scene("clipper: scenes", [&] { Context ctx; ReservedCloud r(ctx, 8); SceneClipperProjective2D c(ctx); c.param_projector.reset(); c.setFullScene(&r); c.compute(); });
  scene("clipper: projector", [&] { Context ctx; ReservedCloud r(ctx, 8), q(ctx, 8); SceneClipperProjective2D c(ctx); c.param_projector.reset(); c.setFullScene(&r); c.setClippedSceneInRobot(&q); c.compute(); });
  failing("clipper: call fails", "lsm2d_clip_scene_voxelized", 1, [&] { Context ctx; ReservedCloud r(ctx, 8), q(ctx, 8); SceneClipperProjective2D c(ctx); c.setFullScene(&r); c.setClippedSceneInRobot(&q); c.compute(); });
  scene("merger: projector", [&] { Context ctx; MergerProjective2D m(ctx); m.param_projector.reset(); m.compute(); });
  scene("merger: scene", [&] { Context ctx; MergerProjective2D m(ctx); m.setMeasurement(&a); m.compute(); });
  scene("merger: measurement", [&] { Context ctx; ReservedCloud r(ctx, 8); MergerProjective2D m(ctx); m.setScene(&r); m.setMeasurement(&a); m.setMeasurement((const PointNormal2fVectorCloud*) nullptr); m.compute(); });
  scene("merger: all, projector", [&] { Context ctx; MergerProjective2D m(ctx); m.param_projector.reset(); m.computeAll({}, {}); });
  scene("merger: all, nothing to merge", [&] { Context ctx; ReservedCloud r(ctx, 8); MergerProjective2D m(ctx); m.setScene(&r); m.computeAll({}, {}); });
  scene("merger: all, a pose each", [&] { Context ctx; ReservedCloud r(ctx, 8), q(ctx, 8); MergerProjective2D m(ctx); m.setScene(&r); m.computeAll({&q}, {POSES[0], POSES[1]}); });
  scene("merger: all, scene", [&] { Context ctx; ReservedCloud q(ctx, 8); MergerProjective2D m(ctx); m.computeAll({&q}, {POSES[0]}); });
  failing("merger: call fails", "lsm2d_merge_scene", 1, [&] { Context ctx; ReservedCloud r(ctx, 8), q(ctx, 8); MergerProjective2D m(ctx); m.setScene(&r); m.setMeasurement(&q); m.compute(); });
  failing("merger: all, call fails", "lsm2d_merge_scenes", 1, [&] { Context ctx; ReservedCloud r(ctx, 8), q(ctx, 8); MergerProjective2D m(ctx); m.setScene(&r); m.computeAll({&q}, {POSES[0]}); });

  const MultiAligner2D::PropertyContainer clouds{{"points", &a}, {"null", nullptr}};
  scene("slice processor: finder", [] { AlignerSliceProcessorLaser2D s; s.sliceParams(); });
  scene("aligner: fixed", [&] { Context ctx; MultiAligner2D al(ctx); al.setMoving(&clouds); al.compute(); });
  scene("aligner: moving", [&] { Context ctx; MultiAligner2D al(ctx); al.setFixed(&clouds); al.compute(); });
  scene("aligner: slice processors", [&] { Context ctx; MultiAligner2D al(ctx); al.setFixed(&clouds); al.setMoving(&clouds); al.compute(); });
  scene("aligner: a processor without a finder", [&] { Context ctx; MultiAligner2D al(ctx); al.setFixed(&clouds); al.setMoving(&clouds); al.param_slice_processors = {std::make_shared<AlignerSliceProcessorLaser2D>()}; al.compute(); });
  for (const char* name : {"rear", "null"})
    scene(std::string("aligner: slice cloud ") + name, [&] { Context ctx; MultiAligner2D al(ctx); al.setFixed(&clouds); al.setMoving(&clouds); al.param_slice_processors = {processor(ctx, "points", false, 0.f), processor(ctx, name, false, 0.f)}; al.compute(); });
  scene("aligner: moving slice cloud", [&] { Context ctx; MultiAligner2D al(ctx); al.setFixed(&clouds); al.setMoving(&clouds); auto p = processor(ctx, "points", false, 0.f); p->param_moving_slice_name = "rear"; al.param_slice_processors = {p}; al.compute(); });
  scene("aligner: correspondences of a slice it has not", [&] { Context ctx; MultiAligner2D al(ctx); al.setFixed(&clouds); al.setMoving(&clouds); al.param_slice_processors = {processor(ctx, "points", false, 0.f)}; al.compute(); al.correspondences(1); });
  for (int store = 0; store < 2; ++store)
    failing(store ? "aligner: pairs call fails" : "aligner: call fails", store ? "lsm2d_align_batch_pairs" : "lsm2d_align_batch", 1, [&] {
      Context ctx; MultiAligner2D al(ctx); al.setFixed(&clouds); al.setMoving(&clouds); al.store_correspondences = store != 0; al.param_slice_processors = {processor(ctx, "points", false, 0.f)}; al.compute(); });
  failing("aligner: second upload fails", "lsm2d_cloudset_create", 2, [&] { Context ctx; MultiAligner2D al(ctx); al.setFixed(&clouds); al.setMoving(&clouds); al.param_slice_processors = {processor(ctx, "points", false, 0.f)}; al.compute(); });

  const lsm2d_preprocessor pre{4, -1.5f, 1.5f, 0.3f, 20.f, 0.3f, 3, 0.02f};
  const std::vector<float> ranges{1.f, 2.f, 3.f, 4.f};
  scene("stream: n_scans", [&] { Sets s; LaserMessageBatchStream st(s.ctx, pre, s.one, sp, ALIGNER, 0); });
  for (int kth = 1; kth <= 3; ++kth)
    failing("stream: create " + std::to_string(kth) + " of the first push fails", "lsm2d_preprocess_scans", kth, [&] { Sets s; LaserMessageBatchStream st(s.ctx, pre, s.one, sp, ALIGNER, 1); st.push(ranges.data(), &POSES[0]); });
  failing("stream: refill fails", "lsm2d_preprocess_scans_refill", 1, [&] { Sets s; LaserMessageBatchStream st(s.ctx, pre, s.one, sp, ALIGNER, 1); for (int k = 0; k < 2; ++k) st.push(ranges.data(), &POSES[0]); });
  failing("stream: begin fails", "lsm2d_align_batch_begin", 2, [&] { Sets s; LaserMessageBatchStream st(s.ctx, pre, s.one, sp, ALIGNER, 1); for (int k = 0; k < 3; ++k) st.push(ranges.data(), &POSES[0]); });
  failing("stream: wait fails", "lsm2d_align_batch_wait", 1, [&] { Sets s; LaserMessageBatchStream st(s.ctx, pre, s.one, sp, ALIGNER, 1); for (int k = 0; k < 4; ++k) st.push(ranges.data(), &POSES[0]); });
  failing("stream: wait fails in a flush", "lsm2d_align_batch_wait", 1, [&] { Sets s; LaserMessageBatchStream st(s.ctx, pre, s.one, sp, ALIGNER, 1); st.push(ranges.data(), &POSES[0]); st.flush(); });

  for (int kth = 1; kth <= 2; ++kth) {
    failing("trackers: create " + std::to_string(kth) + " of the constructor fails", "lsm2d_cloudset_create_reserved_many", kth, [&] { Context ctx; TrackerBatch tb(ctx, 3, trackerParams(0.f)); });
    failing("trackers: preprocess " + std::to_string(kth) + " of reset fails", "lsm2d_preprocess_scans", kth, [&] { Context ctx; TrackerBatch tb(ctx, 3, trackerParams(0.f)); tb.reset(2, BOTH, FRONT, REAR, START); });
    failing("trackers: preprocess " + std::to_string(kth) + " of the first step fails", "lsm2d_preprocess_scans", kth, [&] { Context ctx; TrackerBatch tb(ctx, 3, trackerParams(0.f)); tb.step(FRONT, REAR, ODOMETRY); });
    failing("trackers: refill " + std::to_string(kth) + " of the second step fails", "lsm2d_preprocess_scans_refill", kth, [&] { Context ctx; TrackerBatch tb(ctx, 3, trackerParams(0.f)); for (int k = 0; k < 2; ++k) tb.step(FRONT, REAR, ODOMETRY); });
  }
  for (const char* symbol : {"lsm2d_cloudset_clear_clouds", "lsm2d_merge_scene_batch", "lsm2d_synchronize"})
    failing(std::string("trackers: reset, ") + symbol + " fails", symbol, 1, [&] { Context ctx; TrackerBatch tb(ctx, 3, trackerParams(0.f)); tb.reset(2, BOTH, FRONT, REAR, START); });
  for (const char* symbol : {"lsm2d_clip_scene_batch", "lsm2d_clip_scene_voxelized_batch", "lsm2d_align_batch", "lsm2d_merge_scene_batch"})
    failing(std::string("trackers: step, ") + symbol + " fails", symbol, 1, [&] { Context ctx; TrackerBatch tb(ctx, 3, trackerParams(symbol == std::string("lsm2d_clip_scene_voxelized_batch") ? 0.1f : 0.f)); tb.step(FRONT, REAR, ODOMETRY); });

  failing("sweep: create fails", "lsm2d_sweep_create", 1, [] { LoopClosureSweep sw({0}); });
  scene("sweep: compute, a scan index each", [] { LoopClosureSweep sw({0}); sw.compute({0}, POSES); });
  scene("sweep: computeSelect, a scan index each", [] { LoopClosureSweep sw({0}); sw.computeSelect({0, 1}, POSES, 2); });
  failing("sweep: set_map fails", "lsm2d_sweep_set_map", 1, [&] { LoopClosureSweep sw({0}); sw.setMap(a); });
  failing("sweep: set_scans fails", "lsm2d_sweep_set_scans", 1, [&] { LoopClosureSweep sw({0}); sw.setScans({a, b}); });
  failing("sweep: packed set_scans fails", "lsm2d_sweep_set_scans", 1, [&] { LoopClosureSweep sw({0}); const int32_t offs[2] = {0, 1}; sw.setScansPacked(&a[0].x, offs, 1); });
  failing("sweep: align fails", "lsm2d_sweep_align", 1, [] { LoopClosureSweep sw({0}); sw.compute({0, 0, 0}, POSES); });
  failing("sweep: align_select fails", "lsm2d_sweep_align_select", 1, [] { LoopClosureSweep sw({0}); sw.computeSelect({0, 0, 0}, POSES, 2); });
}

int main() {
  scene("context and cloud sets", contextAndSets);
  scene("finder, factor and score functions", freeFunctions);
  scene("relocalize, one slice", relocalizeOneSlice);
  scene("aligner scores, alignSelect and relocalize", alignerFunctions);
  scene("finder classes", finders);
  scene("clipper and merger", mapping);
  scene("MultiAligner2D", multiAligner);
  scene("LaserMessageBatchStream: five pushes and the flush loop", stream);
  scene("LaserMessageBatchStream: two batches left to the destructor", streamLeftToItsDestructor);
  scene("TrackerBatch: reset and two steps", [] { trackers(0.f); });
  scene("TrackerBatch: reset and two steps, voxelised clip", [] { trackers(0.1f); });
  scene("LoopClosureSweep", sweep);
  refusals();
  fflush(stdout);
  if (g_leaks) fprintf(stderr, "mirror_trace_driver: %d handle(s) leaked\n", g_leaks);
  return g_leaks ? 4 : 0;
}
