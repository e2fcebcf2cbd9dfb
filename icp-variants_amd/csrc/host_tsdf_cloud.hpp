// host_tsdf_cloud.hpp -- icp_tsdf_integrate_cloud: a resident cloud (a laser scan in its sensor frame) fused into the context's TSDF
// volume, dense or hashed, as one observation.  Kernels: dev_tsdf_cloud.hpp; the room rule of the hashed touch: host_tsdf_hash.hpp.
// Free-space carving (icp_set_tsdf_carve_options; kernels: dev_tsdf_carve.hpp) replaces the accumulate launch of
// every cloud fuse while it is on, and nothing else.
// The coloured call (icp_tsdf_integrate_cloud_color; kernels: dev_tsdf_cloud_color.hpp) adds a colour accumulate and a
// colour fold behind the geometry's launches, and nothing else.
// Contract: include/icp_hip.h, DESIGN.md section 6ze.  Part of icp_hip.hip (included from there, after host_tsdf_hash_evict.hpp).
namespace {
// the voxels the accumulators have to cover: every voxel of the pool, or of the box
size_t tsdf_cloud_voxels(const icp_ctx* c) { return c->tsdf_hashed ? (size_t)c->th_pool_cap * 512 : tsdf_voxels(c); }
// The accumulators [S: 8 bytes per voxel | N: 4 bytes per voxel], all zero between calls.  Made and cleared at the first call, and again
// whenever the storage they index has changed its size (growth, create, upload); tc_voxels = 0 while they may hold anything else.
int tsdf_cloud_scratch(icp_ctx* c) {
    const size_t v = tsdf_cloud_voxels(c);
    if (c->tc_acc.p && c->tc_voxels == v) return ICP_OK;
    int rc;
    c->tc_voxels = 0;
    if ((rc = ensure(c, c->tc_acc, v * 12))) return rc;
    HIPCK(c, hipMemsetAsync(c->tc_acc.p, 0, v * 12, c->stream));
    c->tc_voxels = v;
    return ICP_OK;
}
// The colour accumulators [SR | SG | SB | NC: 16 bytes per voxel], all zero between calls: made at the first coloured call and re-made as
// tc_acc is; tcc_voxels = 0 while they may hold anything else.
int tsdf_cloud_color_scratch(icp_ctx* c) {
    const size_t v = tsdf_cloud_voxels(c);
    if (c->tcc_acc.p && c->tcc_voxels == v) return ICP_OK;
    int rc;
    c->tcc_voxels = 0;
    if ((rc = ensure(c, c->tcc_acc, v * 16))) return rc;
    HIPCK(c, hipMemsetAsync(c->tcc_acc.p, 0, v * 16, c->stream));
    c->tcc_voxels = v;
    return ICP_OK;
}
struct TcCall { TcCloud cl; TsdfMat P; float e[3]; TcGrid g; };
constexpr int TCV_MAX_STEPS = 65536;
const char* tsdf_carve_options_error(const icp_tsdf_carve_options* o) {
    if (!o) return "null options";
    if (!(o->distance >= 0.f)) return "distance must be 0 (off), positive or +inf";
    if (!(o->min_range >= 0.f) || !std::isfinite(o->min_range)) return "min_range must be finite and >= 0";
    return nullptr;
}
// J of a cloud fuse with the context's carve options on its volume: 0 = off; beyond the cap the call is refused (no device work yet).
int tsdf_carve_steps(icp_ctx* c, const char* who, int* J) {
    *J = 0;
    if (!(c->tcv_opt.distance > 0.f)) return ICP_OK;
    const double j = std::ceil(std::min((double)c->tcv_opt.distance, (double)c->tsdf_opt.max_depth) / (double)c->tsdf_opt.voxel_size);
    if (!(j <= (double)TCV_MAX_STEPS)) {
        c->err = std::string(who) + ": carving would walk more than 65536 steps per ray (min(distance, max_depth) / voxel_size; icp_set_tsdf_carve_options)";
        return ICP_ERR_INVALID_ARG;
    }
    *J = (int)j;
    return ICP_OK;
}
TcCall tsdf_cloud_call(const icp_ctx* c, const Cloud& cl, const float pose[16], const float* e) {
    const icp_tsdf_options& o = c->tsdf_opt;
    TcCall k;
    k.cl.x = cl.x.as<float>(); k.cl.y = cl.y.as<float>(); k.cl.z = cl.z.as<float>(); k.cl.n = cl.n;
    memcpy(k.P.m, pose, 64);
    for (int a = 0; a < 3; a++) k.e[a] = e ? e[a] : 0.f;
    k.g.ox = o.origin[0]; k.g.oy = o.origin[1]; k.g.oz = o.origin[2]; k.g.s = o.voxel_size; k.g.trunc = o.truncation; k.g.max_d = o.max_depth;
    k.g.n_steps = (int)std::ceil(2.0 * (double)o.truncation / (double)o.voxel_size);
    return k;
}
void tsdf_cloud_touch_launch(icp_ctx* c, const TcCall& k) {
    hipLaunchKernelGGL(k_htsdf_touch_cloud, dim3((k.cl.n + 255) / 256), dim3(256), 0, c->stream, htsdf_table(c), k.cl, k.P, k.e[0], k.e[1], k.e[2], k.g, c->th_ctr.as<int>());
}
void tsdf_cloud_accumulate_launch(icp_ctx* c, const TcCall& k) {
    const size_t v = tsdf_cloud_voxels(c);
    unsigned long long* S = c->tc_acc.as<unsigned long long>();
    int* N = (int*)(c->tc_acc.as<char>() + v * 8);
    unsigned long long* ctr = c->tc_ctr.as<unsigned long long>();
    const dim3 grid((k.cl.n + 255) / 256);
    if (c->tsdf_hashed) hipLaunchKernelGGL(k_htsdf_accumulate_cloud, grid, dim3(256), 0, c->stream, htsdf_view(c), k.cl, k.P, k.e[0], k.e[1], k.e[2], k.g, S, N, ctr);
    else hipLaunchKernelGGL(k_tsdf_accumulate_cloud, grid, dim3(256), 0, c->stream, c->tsdf_opt.dims[0], c->tsdf_opt.dims[1], c->tsdf_opt.dims[2], k.cl, k.P, k.e[0], k.e[1],
                            k.e[2], k.g, S, N, ctr);
}
// The accumulate with the walk started J steps in front of the band.
void tsdf_carve_launch(icp_ctx* c, const TcCall& k, int J) {
    const size_t v = tsdf_cloud_voxels(c);
    unsigned long long* S = c->tc_acc.as<unsigned long long>();
    int* N = (int*)(c->tc_acc.as<char>() + v * 8);
    unsigned long long* ctr = c->tc_ctr.as<unsigned long long>();
    const dim3 grid((k.cl.n + 255) / 256);
    const TcCarve cv = {J, c->tcv_opt.min_range};
    if (c->tsdf_hashed) hipLaunchKernelGGL(k_htsdf_carve_cloud, grid, dim3(256), 0, c->stream, htsdf_view(c), k.cl, k.P, k.e[0], k.e[1], k.e[2], k.g, cv, S, N, ctr);
    else hipLaunchKernelGGL(k_tsdf_carve_cloud, grid, dim3(256), 0, c->stream, c->tsdf_opt.dims[0], c->tsdf_opt.dims[1], c->tsdf_opt.dims[2], k.cl, k.P, k.e[0], k.e[1],
                            k.e[2], k.g, cv, S, N, ctr);
}
void tsdf_cloud_fold_launch(icp_ctx* c) {
    const size_t v = tsdf_cloud_voxels(c);
    const icp_tsdf_options& o = c->tsdf_opt;
    unsigned long long* S = c->tc_acc.as<unsigned long long>();
    int* N = (int*)(c->tc_acc.as<char>() + v * 8);
    unsigned long long* ctr = c->tc_ctr.as<unsigned long long>();
    if (c->tsdf_hashed) {
        if (c->th_nblk > 0) hipLaunchKernelGGL(k_htsdf_fold_cloud, dim3(c->th_nblk), dim3(512), 0, c->stream, c->th_pool.as<float2>(), o.max_weight, S, N, ctr);
    } else {
        const dim3 grid((o.dims[0] + 63) / 64, (o.dims[1] + 3) / 4, (o.dims[2] + TSDF_KCHUNK - 1) / TSDF_KCHUNK);
        hipLaunchKernelGGL(k_tsdf_fold_cloud, grid, dim3(64, 4), 0, c->stream, c->tsdf_vox.as<float2>(), o.dims[0], o.dims[1], o.dims[2], o.max_weight, S, N, ctr);
    }
}
// The colour accumulate behind either geometry accumulate, and the colour fold (the volume is coloured: tsdf_cloud_color_check).
void tsdf_cloud_color_accumulate_launch(icp_ctx* c, const TcCall& k, const Cloud& cl) {
    uint32_t* acc = c->tcc_acc.as<uint32_t>();
    const uint32_t* rgba = cl.rgba.as<uint32_t>();
    const dim3 grid((k.cl.n + 255) / 256);
    if (c->tsdf_hashed) hipLaunchKernelGGL(k_htsdf_accumulate_cloud_color, grid, dim3(256), 0, c->stream, htsdf_view(c), k.cl, rgba, k.P, k.e[0], k.e[1], k.e[2], k.g, acc);
    else hipLaunchKernelGGL(k_tsdf_accumulate_cloud_color, grid, dim3(256), 0, c->stream, c->tsdf_opt.dims[0], c->tsdf_opt.dims[1], c->tsdf_opt.dims[2], k.cl, rgba, k.P, k.e[0],
                            k.e[1], k.e[2], k.g, acc);
}
void tsdf_cloud_color_fold_launch(icp_ctx* c) {
    const icp_tsdf_options& o = c->tsdf_opt;
    uint4* acc = c->tcc_acc.as<uint4>();
    unsigned long long* ctr = c->tc_ctr.as<unsigned long long>();
    if (c->tsdf_hashed) {
        if (c->th_nblk > 0) hipLaunchKernelGGL(k_htsdf_fold_cloud_color, dim3(c->th_nblk), dim3(512), 0, c->stream, c->th_cpool.as<float4>(), o.max_weight, acc, ctr);
    } else {
        const dim3 grid((o.dims[0] + 63) / 64, (o.dims[1] + 3) / 4, (o.dims[2] + TSDF_KCHUNK - 1) / TSDF_KCHUNK);
        hipLaunchKernelGGL(k_tsdf_fold_cloud_color, grid, dim3(64, 4), 0, c->stream, c->tsdf_col.as<float4>(), o.dims[0], o.dims[1], o.dims[2], o.max_weight, acc, ctr);
    }
}
// The checks that need no device, in the order the header states them; *cl_out: the cloud.
int tsdf_cloud_check(icp_ctx* c, int32_t which, const float* pose, const float* e, const char* who, const Cloud** cl_out) {
    if (!c->tsdf_on) { c->err = std::string(who) + ": no volume (icp_tsdf_create, icp_tsdf_create_hashed)"; return ICP_ERR_INVALID_ARG; }
    if ((which != 0 && which != 1) || !pose) { c->err = std::string(who) + ": bad argument (which 0 or 1, pose)"; return ICP_ERR_INVALID_ARG; }
    for (int k = 0; k < 16; k++) if (!std::isfinite(pose[k])) { c->err = std::string(who) + ": the pose must be finite"; return ICP_ERR_INVALID_ARG; }
    if (e) for (int a = 0; a < 3; a++) if (!std::isfinite(e[a])) { c->err = std::string(who) + ": the sensor origin must be finite"; return ICP_ERR_INVALID_ARG; }
    const Cloud& cl = which ? c->src : c->tgt;
    if (cl.n <= 0) {
        c->err = std::string(who) + (which ? ": no source cloud (icp_set_source)" : ": no target cloud (icp_set_target)");
        return which ? ICP_ERR_NO_SOURCE : ICP_ERR_NO_TARGET;
    }
    *cl_out = &cl;
    int J;
    return tsdf_carve_steps(c, who, &J);
}
// The colour checks of the coloured calls, behind the call's own: the volume has colours; the cloud (cl: NULL in the loop, which uploads its
// own) has colours and at most 2^24 points.
bool tsdf_volume_colored(const icp_ctx* c) { return c->tsdf_hashed ? c->th_color : c->tsdf_col_on; }
int tsdf_cloud_color_check(icp_ctx* c, const Cloud* cl, const char* who) {
    if (!tsdf_volume_colored(c)) {
        c->err = std::string(who) + ": the volume has no colours (icp_tsdf_color_create, icp_tsdf_create_color_hashed)";
        return ICP_ERR_INVALID_ARG;
    }
    if (!cl) return ICP_OK;
    if (!cl->has_colors) { c->err = std::string(who) + ": the cloud has no colours (icp_set_target / icp_set_source with rgba)"; return ICP_ERR_COLOR_MISMATCH; }
    if (cl->n > ICP_TSDF_CLOUD_COLOR_MAX_POINTS) { c->err = std::string(who) + ": more than 2^24 points (the colour sums are 32-bit)"; return ICP_ERR_INVALID_ARG; }
    return ICP_OK;
}
// The call behind its checks.  ms (icp_debug_tsdf_cloud_time): after the call, ONE more touch, accumulate and fold launch, each between
// events -- the scan is then fused a second time.  With carving on (J > 0) the accumulate launch is the carving one, and the fifth
// counter, read with the other four, is the call's n_carved.  color: the colour accumulate and the colour fold follow the geometry's fold
// (the two touch different arrays), the sixth counter, read with the other five, is *n_colored_out, and ms has two more times.
int tsdf_cloud_run(icp_ctx* c, const Cloud& cl, const float pose[16], const float* e, icp_tsdf_cloud_info* info_out, const char* who, float* ms, bool color = false,
                   int32_t* n_colored_out = nullptr) {
    int rc, J;
    if ((rc = tsdf_carve_steps(c, who, &J))) return rc;
    const TcCall k = tsdf_cloud_call(c, cl, pose, e);
    const int nctr = color ? TCC_NCTR : TCV_NCTR;
    if ((rc = ensure(c, c->tc_ctr, TCC_NCTR * 8))) return rc;
    if (c->tsdf_hashed) {
        auto touch = [&]() { tsdf_cloud_touch_launch(c, k); return (int)ICP_OK; };
        if ((rc = htsdf_claim(c, touch, who, nullptr))) return rc;      // (a refusal leaves the volume as it was: nothing below has run)
    }
    if ((rc = tsdf_cloud_scratch(c))) return rc;
    if (color && (rc = tsdf_cloud_color_scratch(c))) return rc;
    const size_t v = c->tc_voxels;
    unsigned long long h[TCC_NCTR] = {};
    for (int pass = 0; pass < (ms ? 2 : 1); pass++) {
        HIPCK(c, hipMemsetAsync(c->tc_ctr.p, 0, (size_t)nctr * 8, c->stream));
        c->tc_voxels = 0;                              // (until the fold has zeroed what the accumulate writes)
        if (color) c->tcc_voxels = 0;
        if (pass == 1) {
            if ((rc = ensure_events(c, 6))) return rc;
            HIPCK(c, hipEventRecord(c->events[0], c->stream));
            if (c->tsdf_hashed) tsdf_cloud_touch_launch(c, k);
            HIPCK(c, hipEventRecord(c->events[1], c->stream));
        }
        if (J > 0) tsdf_carve_launch(c, k, J);
        else tsdf_cloud_accumulate_launch(c, k);
        if (pass == 1) HIPCK(c, hipEventRecord(c->events[2], c->stream));
        tsdf_cloud_fold_launch(c);
        if (pass == 1) HIPCK(c, hipEventRecord(c->events[3], c->stream));
        if (color) {
            tsdf_cloud_color_accumulate_launch(c, k, cl);
            if (pass == 1) HIPCK(c, hipEventRecord(c->events[4], c->stream));
            tsdf_cloud_color_fold_launch(c);
            if (pass == 1) HIPCK(c, hipEventRecord(c->events[5], c->stream));
        }
        HIPCK(c, hipGetLastError());
        if ((rc = read_count(c, c->tc_ctr.p, (int*)h, nctr * 2))) return rc;      // (waits)
        c->tc_voxels = v;
        if (color) c->tcc_voxels = v;
        if (c->tsdf_hashed) c->th_oor += (long long)h[TC_OUTSIDE];
        c->tcv_info.n_steps = J; c->tcv_info.n_carved = (int64_t)h[TC_CARVED]; c->tcv_info.n_carved_total += (int64_t)h[TC_CARVED];
    }
    if (ms) {
        for (int q = 0; q < (color ? 5 : 3); q++) HIPCK(c, hipEventElapsedTime(ms + q, c->events[q], c->events[q + 1]));
        if (c->tsdf_hashed) { HIPCK(c, hipMemsetAsync(c->th_ctr.as<int>() + HT_UNPLACED, 0, 8, c->stream)); HIPCK(c, hipStreamSynchronize(c->stream)); }
    }
    if (info_out) {
        info_out->n_points = cl.n; info_out->n_rays = (int32_t)h[TC_RAYS]; info_out->n_updated = (int32_t)h[TC_UPDATED];
        info_out->n_blocks = c->tsdf_hashed ? c->th_nblk : 0;
        info_out->n_samples = (int64_t)h[TC_SAMPLES]; info_out->n_outside = (int64_t)h[TC_OUTSIDE];
    }
    if (n_colored_out) *n_colored_out = (int32_t)h[TCC_COLORED];
    return ICP_OK;
}
}  // namespace

int icp_tsdf_integrate_cloud(icp_ctx* c, int32_t which, const float pose[16], const float sensor_origin[3], icp_tsdf_cloud_info* info_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (info_out) memset(info_out, 0, sizeof(*info_out));
    const char* who = "icp_tsdf_integrate_cloud";
    int rc;
    const Cloud* cl = nullptr;
    if ((rc = tsdf_cloud_check(c, which, pose, sensor_origin, who, &cl))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = tsdf_cloud_run(c, *cl, pose, sensor_origin, info_out, who, nullptr))) return rc;
    return guard.done();
}

int icp_tsdf_integrate_cloud_color(icp_ctx* c, int32_t which, const float pose[16], const float sensor_origin[3], icp_tsdf_cloud_info* info_out, int32_t* n_colored_out) {
    if (!c) return ICP_ERR_INVALID_ARG;
    if (info_out) memset(info_out, 0, sizeof(*info_out));
    if (n_colored_out) *n_colored_out = 0;
    const char* who = "icp_tsdf_integrate_cloud_color";
    int rc;
    const Cloud* cl = nullptr;
    if ((rc = tsdf_cloud_check(c, which, pose, sensor_origin, who, &cl))) return rc;
    if ((rc = tsdf_cloud_color_check(c, cl, who))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = tsdf_cloud_run(c, *cl, pose, sensor_origin, info_out, who, nullptr, true, n_colored_out))) return rc;
    return guard.done();
}

// Not part of icp_hip.h (tools/time_tsdf_cloud.py): icp_tsdf_integrate_cloud, then the device time of ONE touch, ONE accumulate and ONE fold
// launch of the same cloud between events on the context's stream (ms_out[3]; the touch claims nothing new; dense: touch 0).  The scan
// ends up fused twice.
extern "C" int icp_debug_tsdf_cloud_time(icp_ctx* c, int32_t which, const float pose[16], const float sensor_origin[3], float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_tsdf_cloud_time";
    int rc;
    const Cloud* cl = nullptr;
    if ((rc = tsdf_cloud_check(c, which, pose, sensor_origin, who, &cl))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = tsdf_cloud_run(c, *cl, pose, sensor_origin, nullptr, who, ms_out))) return rc;
    return guard.done();
}

// Not part of icp_hip.h (tools/time_tsdf_cloud_color.py): icp_tsdf_integrate_cloud_color, then the device time of ONE touch, ONE accumulate
// (the carving one while carving is on), ONE fold, ONE colour accumulate and ONE colour fold launch of the same cloud between events on the
// context's stream (ms_out[5]).  The scan ends up fused twice, colours included.
extern "C" int icp_debug_tsdf_cloud_color_time(icp_ctx* c, int32_t which, const float pose[16], const float sensor_origin[3], float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    const char* who = "icp_debug_tsdf_cloud_color_time";
    int rc;
    const Cloud* cl = nullptr;
    if ((rc = tsdf_cloud_check(c, which, pose, sensor_origin, who, &cl))) return rc;
    if ((rc = tsdf_cloud_color_check(c, cl, who))) return rc;
    DrainOnError guard(c);
    if ((rc = set_device(c))) return rc;
    if ((rc = tsdf_cloud_run(c, *cl, pose, sensor_origin, nullptr, who, ms_out, true, nullptr))) return rc;
    return guard.done();
}

// ---- free-space carving of the cloud fuses (contract: include/icp_hip.h) ----
int icp_tsdf_carve_options_default(icp_tsdf_carve_options* o) {
    if (!o) return ICP_ERR_INVALID_ARG;
    o->distance = 0.f; o->min_range = 0.f;
    return ICP_OK;
}
int icp_tsdf_carve_options_check(const icp_tsdf_carve_options* o) { return tsdf_carve_options_error(o) ? ICP_ERR_INVALID_ARG : ICP_OK; }
int icp_set_tsdf_carve_options(icp_ctx* c, const icp_tsdf_carve_options* o) {
    if (!c) return ICP_ERR_INVALID_ARG;
    icp_tsdf_carve_options v;
    if (o) v = *o; else icp_tsdf_carve_options_default(&v);
    if (const char* why = tsdf_carve_options_error(&v)) { c->err = std::string("icp_set_tsdf_carve_options: ") + why; return ICP_ERR_INVALID_ARG; }
    c->tcv_opt = v;
    c->tcv_info = icp_tsdf_carve_info{0, 0, 0, 0};
    return ICP_OK;
}
int icp_get_tsdf_carve_options(const icp_ctx* c, icp_tsdf_carve_options* o) { if (!c || !o) return ICP_ERR_INVALID_ARG; *o = c->tcv_opt; return ICP_OK; }
int icp_tsdf_carve_stats(const icp_ctx* c, icp_tsdf_carve_info* out) { if (!c || !out) return ICP_ERR_INVALID_ARG; *out = c->tcv_info; return ICP_OK; }

// Not part of icp_hip.h (tools/time_tsdf_carve.py): icp_debug_tsdf_cloud_time, which times the carving accumulate as its ONE accumulate
// launch while carving is on -- and is refused here while it is off, so that a timing named for carving cannot be the plain launch's.
extern "C" int icp_debug_tsdf_carve_time(icp_ctx* c, int32_t which, const float pose[16], const float sensor_origin[3], float* ms_out) {
    if (!c || !ms_out) return ICP_ERR_INVALID_ARG;
    if (!(c->tcv_opt.distance > 0.f)) { c->err = "icp_debug_tsdf_carve_time: carving is off"; return ICP_ERR_INVALID_ARG; }
    return icp_debug_tsdf_cloud_time(c, which, pose, sensor_origin, ms_out);
}
