// lsm2d_capi_cloudsets.inc -- cloud sets: device-resident ragged batches of PointNormal2fVectorCloud (create, reserve, upload, download, pending sizes and deferred unpacking).
// Part of lsm2d_capi.hip (included there); not a translation unit of its own.
// ---- cloud sets -----------------------------------------------------------------------------------
static int cloudset_layout(lsm2d_cloudset* cs, const int32_t* offsets, int32_t n_clouds, int64_t total) {
  cs->n_clouds = n_clouds; cs->total = total;
  cs->h_start.resize(n_clouds); cs->h_count.resize(n_clouds);
  int64_t p = 0;
  for (int32_t c = 0; c < n_clouds; ++c) {
    const int64_t b = offsets ? offsets[c] : 0, e = offsets ? offsets[c + 1] : total;
    if (b < 0 || e < b || e > total) return LSM2D_BAD_ARGUMENT;
    cs->h_start[c] = (int32_t) p; cs->h_count[c] = (int32_t) (e - b);
    p += (e - b); p += (p & 1);        // every cloud starts on an even point index (16-byte aligned xy)
    if (p > 0x7fffffff - 2) return LSM2D_CAPACITY_EXCEEDED;
  }
  if (offsets && (offsets[0] != 0 || offsets[n_clouds] != total)) return LSM2D_BAD_ARGUMENT;
  cs->padded_total = p + 2;            // slack so the last lane's 16-byte load stays in bounds
  return LSM2D_SUCCESS;
}

static int cloudset_alloc(lsm2d_context* ctx, lsm2d_cloudset* cs) {
  HIPCHK(ctx, cs->d_xy.alloc(sizeof(float2) * (size_t) cs->padded_total));
  HIPCHK(ctx, cs->d_nrm.alloc(sizeof(float2) * (size_t) cs->padded_total));
  HIPCHK(ctx, cs->d_start.alloc(sizeof(int32_t) * (size_t) cs->n_clouds));
  HIPCHK(ctx, cs->d_count.alloc(sizeof(int32_t) * (size_t) cs->n_clouds));
  HIPCHK(ctx, hipMemsetAsync(cs->d_xy, 0, sizeof(float2) * (size_t) cs->padded_total, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(cs->d_nrm, 0, sizeof(float2) * (size_t) cs->padded_total, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(cs->d_start, cs->h_start.data(), sizeof(int32_t) * (size_t) cs->n_clouds, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(cs->d_count, cs->h_count.data(), sizeof(int32_t) * (size_t) cs->n_clouds, hipMemcpyHostToDevice, ctx->stream));
  return LSM2D_SUCCESS;
}

// A set under construction: destroyed by whatever return comes before it is released into the caller's `*out`
struct CloudsetDestroy { void operator()(lsm2d_cloudset* cs) const { lsm2d_cloudset_destroy(cs); } };
typedef std::unique_ptr<lsm2d_cloudset, CloudsetDestroy> CloudsetGuard;
// THE way a set comes to be: new, registered with its context (live_sets), laid out by `layout(set)` -- clouds, starts, sizes, padded_total --, allocated
template <class Layout> static int cloudset_new(lsm2d_context* ctx, CloudsetGuard& cs, Layout layout) {
  cs.reset(new (std::nothrow) lsm2d_cloudset);
  if (!cs) return LSM2D_OUT_OF_MEMORY;
  cs->ctx = ctx; ctx->live_sets.push_back(cs.get());
  const int rc = layout(cs.get());
  return rc != LSM2D_SUCCESS ? rc : cloudset_alloc(ctx, cs.get());
}
// ... in fixed slots of `stride` points: n_clouds empty clouds (the reserved forms, a set of scans)
static void cloudset_slots(lsm2d_cloudset* cs, int32_t n_clouds, int64_t stride) {
  cs->n_clouds = n_clouds; cs->total = 0; cs->padded_total = stride * n_clouds + 2;
  cs->h_start.resize(n_clouds); cs->h_count.assign(n_clouds, 0);
  for (int32_t c = 0; c < n_clouds; ++c) cs->h_start[c] = (int32_t) (stride * c);
}

static int cloudset_create_impl(lsm2d_context* ctx, const void* points, bool on_device, const int32_t* offsets,
                                int32_t n_clouds, int64_t total, lsm2d_cloudset** out) {
  if (!ctx || !out || n_clouds < 1 || total < 0 || (total > 0 && !points) || (n_clouds > 1 && !offsets))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "cloudset_create: bad argument");
  *out = nullptr;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  CloudsetGuard cs;
  { const int rc = cloudset_new(ctx, cs, [&](lsm2d_cloudset* s) { return cloudset_layout(s, offsets, n_clouds, total); }); if (rc != LSM2D_SUCCESS) return rc; }
  // (the staging buffers and the one-cloud offsets live until the function returns: behind the wait below, which their copies and the kernel need)
  DevBuf<> d_src; DevBuf<int32_t> d_off;
  const std::vector<int32_t> one = {0, (int32_t) total};
  if (total > 0) {
    // stage the AoS points (and the logical offsets) on the device, then split / pad with one kernel
    const size_t pts_bytes = sizeof(float4) * (size_t) total, off_bytes = sizeof(int32_t) * (size_t) (n_clouds + 1);
    const int32_t* h_off = offsets ? offsets : one.data();
    if (!on_device) {
      ++ctx->uploads; ctx->last_h2d_bytes = (long long) pts_bytes;
      HIPCHK(ctx, d_src.alloc(pts_bytes));
      HIPCHK(ctx, hipMemcpyAsync(d_src, points, pts_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, d_off.alloc(off_bytes));
    HIPCHK(ctx, hipMemcpyAsync(d_off, h_off, off_bytes, hipMemcpyHostToDevice, ctx->stream));
    const int block = 256;
    long long blocks = (total + block - 1) / block; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_repack_cloud, dim3((unsigned) blocks), dim3(block), 0, ctx->stream,
                       (const float4*) (on_device ? points : d_src), d_off, cs->d_start, n_clouds, (long long) total, cs->d_xy, cs->d_nrm);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, stream_sync(ctx));      // (the temporaries above and the caller's points back the copies: they go after this wait)
  *out = cs.release();
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_cloudset_create(lsm2d_context* ctx, const float* pts, const int32_t* offsets, int32_t n_clouds,
                                     int64_t total, lsm2d_cloudset** out) {
  return cloudset_create_impl(ctx, pts, false, offsets, n_clouds, total, out);
}
extern "C" int lsm2d_cloudset_create_from_device(lsm2d_context* ctx, const void* d_pts, const int32_t* offsets,
                                                 int32_t n_clouds, int64_t total, lsm2d_cloudset** out) {
  return cloudset_create_impl(ctx, d_pts, true, offsets, n_clouds, total, out);
}
extern "C" void lsm2d_cloudset_destroy(lsm2d_cloudset* cs) {
  if (!cs) return;
  if (cs->ctx) (void) hipSetDevice(cs->ctx->device);
  if (cs->ctx && cs->staged_epoch == cs->ctx->sync_epoch) (void) stream_sync(cs->ctx);      // a staged transfer may still be reading h_upload
  if (cs->ctx) { auto& v = cs->ctx->live_sets; for (size_t i = 0; i < v.size(); ++i) if (v[i] == cs) { v[i] = v.back(); v.pop_back(); break; } }
  delete cs;      // (its arrays, events, caches and pinned buffer go with it)
}
static int flush_pending(const lsm2d_cloudset* cs);
static int resolve_count(const lsm2d_cloudset* cs) {
  if (!cs || !cs->count_pending) return LSM2D_SUCCESS;
  if (!cs->ctx) return LSM2D_BAD_ARGUMENT;      // its context is gone
  { const int rc0 = flush_pending(cs); if (rc0) return rc0; }      // a preprocessing launch still pending: its result is the count asked for
  lsm2d_context* ctx = cs->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, sync_streams(ctx, false));      // (the side streams: a refill queued on the refill stream; not the lanes' streams: a batch in flight changes no set's size)
  if (cs->n_clouds > 1) {      // a refilled set of scans (lsm2d_preprocess_scans_refill): every cloud's size
    HIPCHK(ctx, hipMemcpy(cs->h_count.data(), cs->d_count, sizeof(int32_t) * (size_t) cs->n_clouds, hipMemcpyDeviceToHost));
    cs->total = 0; for (int c = 0; c < cs->n_clouds; ++c) cs->total += cs->h_count[c];
    cs->count_pending = false;
    return LSM2D_SUCCESS;
  }
  int32_t n = 0;
  HIPCHK(ctx, hipMemcpy(&n, cs->d_count, sizeof(int32_t), hipMemcpyDeviceToHost));
  cs->h_count[0] = n; cs->total = n; cs->count_pending = false;
  return LSM2D_SUCCESS;
}
// queues the unpacking of a set whose latest upload still sits in its pinned buffer; every reader of the device arrays calls it
static int flush_pending(const lsm2d_cloudset* cs) {
  if (cs && !cs->ctx) return LSM2D_BAD_ARGUMENT;      // its context is gone
  if (cs && cs->prep_pending) {
    lsm2d_context* ctx = cs->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_preprocess_scans, dim3(1), dim3(kPrepBlock), 0, ctx->stream, cs->prep_args);
    HIPCHK(ctx, hipGetLastError());
    cs->prep_pending = false; cs->staged_epoch = ctx->sync_epoch;
    return LSM2D_SUCCESS;
  }
  if (!cs || !cs->unpack_pending) return LSM2D_SUCCESS;
  lsm2d_context* ctx = cs->ctx;
  const int n = cs->h_count[0];
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_upload_unpack, dim3((unsigned) (n > 4096 ? 16 : (n + 255) / 256 > 0 ? (n + 255) / 256 : 1)), dim3(256), 0, ctx->stream,
                     (const float4*) cs->h_upload.dev(), n, cs->d_xy, cs->d_nrm, cs->d_count);
  HIPCHK(ctx, hipGetLastError());
  cs->unpack_pending = false; cs->staged_epoch = ctx->sync_epoch;
  return LSM2D_SUCCESS;
}
// the sets an aligner call reads: pending preprocessing launches go out together, one workgroup per scan
static int flush_preprocessing_together(lsm2d_context* ctx, const lsm2d_cloudset* const* sets, int n_sets) {
  const lsm2d_cloudset* todo[kPrepMulti]; int nt = 0;
  for (int i = 0; i < n_sets; ++i) {
    const lsm2d_cloudset* cs = sets[i];
    if (!cs || !cs->prep_pending) continue;
    if (cs->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "cloud set from another (or a destroyed) context");
    bool seen = false; for (int k = 0; k < nt; ++k) seen = seen || todo[k] == cs;
    if (seen) continue;
    if (nt == kPrepMulti) { const int rc = flush_pending(cs); if (rc) return rc; continue; }
    todo[nt++] = cs;
  }
  if (nt == 0) return LSM2D_SUCCESS;
  if (nt == 1) return flush_pending(todo[0]);
  PrepMultiArgs M;
  for (int k = 0; k < nt; ++k) M.a[k] = todo[k]->prep_args;
  for (int k = nt; k < kPrepMulti; ++k) M.a[k] = todo[0]->prep_args;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_preprocess_multi, dim3((unsigned) nt), dim3(kPrepBlock), 0, ctx->stream, M);
  HIPCHK(ctx, hipGetLastError());
  for (int k = 0; k < nt; ++k) { todo[k]->prep_pending = false; todo[k]->staged_epoch = ctx->sync_epoch; }
  return LSM2D_SUCCESS;
}
extern "C" int32_t lsm2d_cloudset_num_clouds(const lsm2d_cloudset* cs) { return cs ? cs->n_clouds : 0; }
extern "C" int64_t lsm2d_cloudset_num_points(const lsm2d_cloudset* cs) { return (cs && resolve_count(cs) == LSM2D_SUCCESS) ? cs->total : 0; }
extern "C" int64_t lsm2d_cloudset_cloud_size(const lsm2d_cloudset* cs, int32_t i) {
  return (cs && i >= 0 && i < cs->n_clouds && resolve_count(cs) == LSM2D_SUCCESS) ? cs->h_count[i] : -1;
}

extern "C" int32_t lsm2d_cloudset_cloud_sizes(const lsm2d_cloudset* cs, int32_t* out, int32_t capacity) {
  if (!cs || capacity < 0 || (capacity > 0 && !out)) return LSM2D_BAD_ARGUMENT;
  const int rc = resolve_count(cs); if (rc != LSM2D_SUCCESS) return rc;
  const int32_t n = capacity < cs->n_clouds ? capacity : cs->n_clouds;
  for (int32_t i = 0; i < n; ++i) out[i] = cs->h_count[(size_t) i];
  return n;
}

// the contents changed: everything derived from them is stale and goes.  Two things stay: a reserved single-cloud set with one KD-tree keeps that tree's
// allocation for the next build (KdCache::valid), and a refill keeps the AoS rows, which its launch rewrites in place (keep_aos)
static void cloudset_drop_grids(const lsm2d_cloudset* cs, bool keep_aos = false) {
  ++cs->version;
  lsm2d_cloudset::Derived fresh;
  if (keep_aos) fresh.d_aos = std::move(cs->derived.d_aos);
  if (cs->capacity > 0 && cs->n_clouds == 1 && cs->derived.kds.size() == 1) { cs->derived.kds[0].valid = false; fresh.kds = std::move(cs->derived.kds); }
  cs->derived = std::move(fresh);
}

// the reserved forms: n_clouds empty clouds with room for `capacity` points each, every slot starting on an even point (16-byte aligned xy), as cloudset_layout lays them out
static int cloudset_create_slots(lsm2d_context* ctx, int32_t n_clouds, int64_t capacity, bool many, lsm2d_cloudset** out) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  CloudsetGuard cs;
  const int rc = cloudset_new(ctx, cs, [&](lsm2d_cloudset* s) { cloudset_slots(s, n_clouds, capacity + (capacity & 1)); s->capacity = capacity; s->many = many; return LSM2D_SUCCESS; });
  if (rc != LSM2D_SUCCESS) return rc;
  if (stream_sync(ctx) != hipSuccess) return LSM2D_DEVICE_ERROR;
  *out = cs.release();
  return LSM2D_SUCCESS;
}
extern "C" int lsm2d_cloudset_create_reserved(lsm2d_context* ctx, int64_t capacity, lsm2d_cloudset** out) {
  if (!ctx || !out || capacity < 1 || capacity > 0x7ffffff0) return fail(ctx, LSM2D_BAD_ARGUMENT, "cloudset_create_reserved: bad argument");
  *out = nullptr;
  return cloudset_create_slots(ctx, 1, capacity, false, out);
}
extern "C" int lsm2d_cloudset_create_reserved_many(lsm2d_context* ctx, int32_t n_clouds, int64_t capacity, lsm2d_cloudset** out) {
  if (!ctx || !out || n_clouds < 1 || capacity < 1 || capacity > 0x7ffffff0) return fail(ctx, LSM2D_BAD_ARGUMENT, "cloudset_create_reserved_many: bad argument");
  *out = nullptr;
  if ((capacity + (capacity & 1)) * n_clouds > 0x7ffffff0) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "cloudset_create_reserved_many: too many points");
  return cloudset_create_slots(ctx, n_clouds, capacity, true, out);
}

// asynchronous: the device-side sizes of the named clouds are zeroed on the context's stream (contiguous runs of indices: one memset each)
extern "C" int lsm2d_cloudset_clear_clouds(lsm2d_cloudset* cs, int32_t n, const int32_t* idx) {
  lsm2d_context* ctx = cs ? cs->ctx : nullptr;
  if (!cs || !ctx || !cs->many || (idx && n < 0)) return fail(ctx, LSM2D_BAD_ARGUMENT, "cloudset_clear_clouds: bad argument");
  const int32_t m = idx ? n : cs->n_clouds;
  for (int32_t k = 0; k < m; ++k) if (idx && (idx[k] < 0 || idx[k] >= cs->n_clouds)) return fail(ctx, LSM2D_BAD_ARGUMENT, "cloudset_clear_clouds: cloud index out of range");
  if (m == 0) return LSM2D_SUCCESS;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, join_refill_stream(ctx, ctx->stream));
  cloudset_drop_grids(cs);
  for (int32_t k = 0; k < m;) {
    const int32_t c0 = idx ? idx[k] : k;
    int32_t len = 1;
    while (k + len < m && (idx ? idx[k + len] : k + len) == c0 + len) ++len;
    HIPCHK(ctx, hipMemsetAsync(cs->d_count + c0, 0, sizeof(int32_t) * (size_t) len, ctx->stream));
    for (int32_t c = c0; c < c0 + len; ++c) { cs->total -= cs->h_count[c]; cs->h_count[c] = 0; }      // exact zeros (the others stay what they were: sizes or bounds)
    k += len;
  }
  return LSM2D_SUCCESS;
}

static int set_single_count(lsm2d_context* ctx, lsm2d_cloudset* cs, int32_t n) {
  cs->h_count[0] = n; cs->total = n;
  HIPCHK(ctx, hipMemcpyAsync(cs->d_count, cs->h_count.data(), sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  return LSM2D_SUCCESS;
}

// the set's own pinned staging buffer, free to be overwritten: waits for the set's previous staged transfer only
static int acquire_upload_stage(lsm2d_cloudset* cs, size_t need) {
  lsm2d_context* ctx = cs->ctx;
  // free to overwrite once the stream has been waited for since the last staged transfer was queued (the aligner call in between
  // does that); two uploads to the same set back to back wait here
  if (cs->staged_epoch == ctx->sync_epoch) HIPCHK(ctx, stream_sync(ctx));
  // ... and a copy queued on a side stream (the refill while a batch is in flight) is not covered by the context stream's epoch: its own event
  if (cs->stage_on_side) { HIPCHK(ctx, hipEventSynchronize(cs->ev_stage)); cs->stage_on_side = false; }
  // (a set of many clouds stages the batched calls' per-tracker arguments only; nothing to wait for here: the waits above cover the old buffer)
  const size_t want = cs->capacity > 0 && !cs->many ? sizeof(float) * 4 * (size_t) cs->capacity + 16 : need;
  HIPCHK(ctx, cs->h_upload.ensure(need, want > need ? want : need, [] { return hipSuccess; }, hipHostMallocCoherent | hipHostMallocMapped));
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_cloudset_upload(lsm2d_cloudset* cs, const float* pts, int64_t n) {
  if (!cs || !cs->ctx || cs->n_clouds != 1 || cs->many || n < 0 || (n > 0 && !pts)) return fail(cs ? cs->ctx : nullptr, LSM2D_BAD_ARGUMENT, "cloudset_upload: bad argument");
  lsm2d_context* ctx = cs->ctx;
  const int64_t cap = cs->capacity > 0 ? cs->capacity : cs->padded_total - 2;
  if (n > cap) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "cloudset_upload: does not fit the allocation");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  cloudset_drop_grids(cs);
  ++ctx->uploads; ctx->last_h2d_bytes = (long long) (sizeof(float) * 4 * (size_t) n);
  // no allocation and no wait for the stream -- only for this set's PREVIOUS upload (an event), whose source the staging buffer
  // still is until it ran
  { const int rc0 = acquire_upload_stage(cs, sizeof(float) * 4 * (size_t) (n > 0 ? n : 1) + 16); if (rc0) return rc0; }
  cs->count_pending = false; cs->prep_pending = false;
  cs->h_count[0] = (int32_t) n; cs->total = n;
  if (n <= 16384) {
    // scan-sized: the points go into the pinned buffer as they are and ONE small kernel reads them over the bus, splits them into
    // the coordinate / normal arrays and sets the count (three host-to-device copies cost three times the API and launch overhead)
    // -- queued by the set's first reader (flush_pending), or done by the aligner kernel itself
    if (n) memcpy(cs->h_upload, pts, sizeof(float) * 4 * (size_t) n);
    cs->unpack_pending = true;
    return LSM2D_SUCCESS;
  } else {
    cs->unpack_pending = false;
    // split on the host, then plain async copies
    float2* hxy = (float2*) cs->h_upload; float2* hn = hxy + n;
    for (int64_t i = 0; i < n; ++i) { hxy[i] = make_float2(pts[4 * i], pts[4 * i + 1]); hn[i] = make_float2(pts[4 * i + 2], pts[4 * i + 3]); }
    if (n) {
      HIPCHK(ctx, hipMemcpyAsync(cs->d_xy, hxy, sizeof(float2) * (size_t) n, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(ctx, hipMemcpyAsync(cs->d_nrm, hn, sizeof(float2) * (size_t) n, hipMemcpyHostToDevice, ctx->stream));
    }
    // the count travels in the same staging buffer (h_count may be rewritten by the host before the copy runs)
    int32_t* hcnt = (int32_t*) ((char*) cs->h_upload + cs->h_upload.bytes - sizeof(int32_t));
    *hcnt = (int32_t) n;
    HIPCHK(ctx, hipMemcpyAsync(cs->d_count, hcnt, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  }
  cs->staged_epoch = ctx->sync_epoch;
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_cloudset_download(const lsm2d_cloudset* cs, int32_t ci, float* out, int64_t capacity, int64_t* out_n) {
  if (!cs || !cs->ctx || !out_n || !valid_cloud_index_fwd(cs, ci)) return fail(cs ? cs->ctx : nullptr, LSM2D_BAD_ARGUMENT, "cloudset_download: bad argument");
  lsm2d_context* ctx = cs->ctx;
  { int rc0 = resolve_count(cs); if (rc0) return rc0; rc0 = flush_pending(cs); if (rc0) return rc0; }
  const int64_t n = cs->h_count[ci];
  *out_n = n;
  if (n > capacity || (n > 0 && !out)) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "cloudset_download: out buffer too small");
  if (n == 0) return LSM2D_SUCCESS;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = sizeof(float4) * (size_t) n;
  int rc = ensure_scratch(ctx, bytes); if (rc) return rc;
  rc = ensure_stage(ctx, bytes); if (rc) return rc;
  Lane& L = lane(ctx);
  const int base = cs->h_start[ci];
  hipLaunchKernelGGL(k_pack_aos, dim3((unsigned) ((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const float2*) (cs->d_xy + base), (const float2*) (cs->d_nrm + base), (int) n, (float4*) L.d_scratch);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(L.h_stage, L.d_scratch, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, stream_sync(ctx));
  memcpy(out, L.h_stage, bytes);
  return LSM2D_SUCCESS;
}
