// WaveFieldRenderer (fgs_wave_*: plan, per-image maximum, output stage and its backward).  The splat itself --
// k_asm_splat<BWD, WAVE = true, NP> -- the phasor table and the per-image reductions are shared with the angular-spectrum
// renderer and live in fgs_splat.h; nothing of that renderer's transfer functions or transforms (fgs_asm.hip) is used here.
// (Not to be confused with fgs_wave.h: wave64 lane helpers.)
//
// Compiled with the flags of fgs_asm.hip (build.py SPLAT_FLAGS): no fast-math, no FMA contraction, no SLP vectoriser.
#include "fgs_splat.h"

namespace {

// the phasor table in a launch of its own (the angular-spectrum renderer fills it inside k_asm_prep)
__global__ __launch_bounds__(256) void k_asm_phasors(uint32_t total, int phase_channels, const float *__restrict__ color,
                                                     const float *__restrict__ phase, float *__restrict__ ccs) {
    asm_phasors_block(blockIdx.x, total, phase_channels, color, phase, ccs);
}

// ---------------------------------------------------------------------------------------------
// WaveFieldRenderer (DR:689-926): order-independent complex accumulation without
// depth planes or propagation; intensity -> sqrt -> per-image max normalisation -> background
// where the total amplitude is low; depth map = sum(a depth) / (sum a + 1e-8).
// ---------------------------------------------------------------------------------------------
struct WavePix {
    float r[3], n[3], v[3], tasq, ta, M;
};

__device__ __forceinline__ void wave_pixel_forward(const float2 u[3], float maxval, const float bg[3], WavePix &o) {
    o.M = maxval < 1.0f ? 1.0f : maxval;
    float isum = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float I = u[c].x * u[c].x + u[c].y * u[c].y;
        isum += I;
        o.r[c] = sqrtf(I + 1e-8f);                           // DR:898
        const float q = o.r[c] / o.M;                        // DR:902-905
        o.n[c] = q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q);
    }
    o.tasq = sqrtf(isum + 1e-8f);                            // DR:908
    o.ta = o.tasq < 0.0f ? 0.0f : (o.tasq > 1.0f ? 1.0f : o.tasq);
#pragma unroll
    for (int c = 0; c < 3; ++c) o.v[c] = o.n[c] + bg[c] * (1.0f - o.ta);
}

__global__ __launch_bounds__(256) void k_wave_max(size_t HW, const float2 *__restrict__ field, float *__restrict__ pmax) {
    const int b = blockIdx.y;
    float mx = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < 3 * HW; i += (size_t)gridDim.x * 256) {
        const float2 u = field[(size_t)b * 3 * HW + i];
        mx = fmaxf(mx, sqrtf(u.x * u.x + u.y * u.y + 1e-8f));
    }
    mx = block_max_256(mx);
    if (threadIdx.x == 0) pmax[(size_t)b * RED_BLOCKS + blockIdx.x] = mx;
}

__global__ __launch_bounds__(256) void k_wave_output(size_t HW, float bg0, float bg1, float bg2,
                                                     const float2 *__restrict__ field, const float2 *__restrict__ dw,
                                                     const float *__restrict__ pmax, float *__restrict__ scal,
                                                     float *__restrict__ out, float *__restrict__ out_depth,
                                                     const uint32_t *__restrict__ seg_off, uint32_t lists_per_image) {
    const int b = blockIdx.y;
    const float maxval = image_max(pmax, b);
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[b] = maxval;  // kept for the backward
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const float bg[3] = {bg0, bg1, bg2};
    if (asm_plane_empty(seg_off, (uint32_t)b, lists_per_image)) {  // no visible Gaussian: plain background, zero depth (DR:801-808)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[((size_t)b * 3 + c) * HW + i] = bg[c];
        out_depth[(size_t)b * HW + i] = 0.0f;
        return;
    }
    const float2 u[3] = {field[((size_t)b * 3 + 0) * HW + i], field[((size_t)b * 3 + 1) * HW + i],
                         field[((size_t)b * 3 + 2) * HW + i]};
    WavePix o;
    wave_pixel_forward(u, maxval, bg, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = o.v[c];
        out[((size_t)b * 3 + c) * HW + i] = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    }
    const float2 d = dw[(size_t)b * HW + i];
    out_depth[(size_t)b * HW + i] = d.x / (d.y + 1e-8f);      // DR:924
}

__global__ __launch_bounds__(256) void k_wave_output_bwd1(size_t HW, float bg0, float bg1, float bg2,
                                                          const float2 *__restrict__ field, const float *__restrict__ scal,
                                                          const float *__restrict__ g_out, float2 *__restrict__ psum) {
    const int b = blockIdx.y;
    float gM = 0.0f, cnt = 0.0f;
    const float bg[3] = {bg0, bg1, bg2};
    const float maxval = scal[b];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
        const float2 u[3] = {field[((size_t)b * 3 + 0) * HW + i], field[((size_t)b * 3 + 1) * HW + i],
                             field[((size_t)b * 3 + 2) * HW + i]};
        WavePix o;
        wave_pixel_forward(u, maxval, bg, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gv = (o.v[c] >= 0.0f && o.v[c] <= 1.0f) ? g_out[((size_t)b * 3 + c) * HW + i] : 0.0f;
            const float q = o.r[c] / o.M;
            const float gq = (q >= 0.0f && q <= 1.0f) ? gv : 0.0f;
            gM -= gq * o.r[c] / (o.M * o.M);
            if (o.r[c] == maxval) cnt += 1.0f;
        }
    }
    const float2 t = block_sum2_256(gM, cnt);
    if (threadIdx.x == 0) psum[(size_t)b * RED_BLOCKS + blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void k_wave_output_bwd2(size_t HW, float bg0, float bg1, float bg2,
                                                          const float2 *__restrict__ field,
                                                          const float2 *__restrict__ dw, const float *__restrict__ scal,
                                                          const float2 *__restrict__ psum,
                                                          const float *__restrict__ g_out,
                                                          const float *__restrict__ g_depth, float2 *__restrict__ gfield,
                                                          float2 *__restrict__ gdw) {
    const int b = blockIdx.y;
    const float2 sums = image_sums(psum, b);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const float2 u[3] = {field[((size_t)b * 3 + 0) * HW + i], field[((size_t)b * 3 + 1) * HW + i],
                         field[((size_t)b * 3 + 2) * HW + i]};
    const float bg[3] = {bg0, bg1, bg2};
    const float maxval = scal[b];
    const float cntm = sums.y;
    const float gMshare = (maxval >= 1.0f && cntm > 0.0f) ? sums.x / cntm : 0.0f;
    WavePix o;
    wave_pixel_forward(u, maxval, bg, o);
    float gv[3], gta = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gv[c] = (o.v[c] >= 0.0f && o.v[c] <= 1.0f) ? g_out[((size_t)b * 3 + c) * HW + i] : 0.0f;
        gta -= gv[c] * bg[c];
    }
    // ta = clamp(sqrt(sum_c I_c + 1e-8), 0, 1): d ta / d I_c = 1 / (2 tasq) inside the clamp
    const float gIsum = (o.tasq >= 0.0f && o.tasq <= 1.0f) ? gta / (2.0f * o.tasq) : 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float q = o.r[c] / o.M;
        float gr = ((q >= 0.0f && q <= 1.0f) ? gv[c] : 0.0f) / o.M;
        if (o.r[c] == maxval) gr += gMshare;
        const float gI = gr / (2.0f * o.r[c]) + gIsum;
        gfield[((size_t)b * 3 + c) * HW + i] = make_float2(2.0f * gI * u[c].x, 2.0f * gI * u[c].y);
    }
    // depth_map = Ad / (Wt + 1e-8)
    const float2 d = dw[(size_t)b * HW + i];
    const float gdm = g_depth[(size_t)b * HW + i];
    const float den = d.y + 1e-8f;
    gdw[(size_t)b * HW + i] = make_float2(gdm / den, -gdm * d.x / (den * den));
}

struct WavePlan {
    FgsWaveDims w;
    FgsPlan base;
    size_t HW, v_field, v_dw, v_scal, v_ccs, v_total_bytes, c_gfield, c_gdw, c_rows, c_part, c_total_bytes;
};

int make_wave_plan(const FgsWaveDims *w, WavePlan *p) {
    if (!w) { fgs_set_error("null dims"); return FGS_EINVAL; }
    if (w->phase_channels != 1 && w->phase_channels != 3) { fgs_set_error("invalid phase_channels"); return FGS_EINVAL; }
    const FgsDims d = splat_base_dims(w->batch, w->num_gaussians, w->width, w->height, w->max_radius, w->background,
                                      w->num_cameras, FGS_TUNE_AUTO);
    p->w = *w;
    const int rc = fgs_make_plan(&d, &p->base, 1, false);
    if (rc) return rc;
    const size_t B = w->batch, HW = (size_t)w->width * w->height;
    p->HW = HW;
    size_t o = p->base.L.total_bytes;
    p->v_field = o; o = align256(o + B * 3 * HW * 8);
    p->v_dw = o; o = align256(o + B * HW * 8);
    p->v_scal = o; o = align256(o + B * 4 * 4);
    p->v_ccs = o; o = align256(o + B * (size_t)w->num_gaussians * 8 * 4);
    p->v_total_bytes = o;
    o = p->base.s_total;
    p->c_gfield = o; o = align256(o + B * 3 * HW * 8);
    p->c_gdw = o; o = align256(o + B * HW * 8);
    p->c_rows = o; o = align256(o + p->base.L.dup_capacity * 16 * 4);
    p->c_part = o; o = align256(o + B * RED_BLOCKS * 8);  // float2 [B][RED_BLOCKS] block partials of the per-image scalars
    p->c_total_bytes = o;
    return FGS_OK;
}

}  // namespace

extern "C" {

int fgs_wave_workspace_bytes(const FgsWaveDims *dims, size_t *saved_bytes, size_t *scratch_bytes) {
    WavePlan p;
    const int rc = make_wave_plan(dims, &p);
    if (rc) return rc;
    if (saved_bytes) *saved_bytes = p.v_total_bytes;
    if (scratch_bytes) *scratch_bytes = p.c_total_bytes;
    return FGS_OK;
}

int fgs_wave_forward(const FgsWaveDims *dims, const float *cameras, const float *pos, const float *scale,
                     const float *quat, const float *color, const float *opacity, const float *phase,
                     float *out_rgb, float *out_depth, void *saved, void *scratch, void *stream) {
    WavePlan p;
    int rc = make_wave_plan(dims, &p);
    if (rc) return rc;
    const void *ptrs[] = {cameras, pos, scale, quat, color, opacity, phase, out_rgb, out_depth, saved, scratch};
    if ((rc = check_ptrs(ptrs, 11, "fgs_wave_forward"))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *sv = reinterpret_cast<char *>(saved), *sc = reinterpret_cast<char *>(scratch);
    const int B = p.w.batch;
    const size_t HW = p.HW;
    fgs_stage_begin(ST_PROJECT, st);
    if ((rc = fgs_launch_project(p.base, cameras, pos, scale, quat, color, opacity, sv, st))) return rc;
    fgs_stage_end(ST_PROJECT, st);
    if ((rc = fgs_launch_binning(p.base, sv, sc, st))) return rc;
    fgs_stage_begin(ST_SPLAT_FWD, st);
    float2 *field = reinterpret_cast<float2 *>(sv + p.v_field);
    float2 *dw = reinterpret_cast<float2 *>(sv + p.v_dw);
    float *scal = reinterpret_cast<float *>(sv + p.v_scal);
    float *ccs = reinterpret_cast<float *>(sv + p.v_ccs);
    const uint32_t ngauss = (uint32_t)B * (uint32_t)p.w.num_gaussians;
    hipLaunchKernelGGL(k_asm_phasors, dim3((ngauss + 255) / 256), dim3(256), 0, st, ngauss, p.w.phase_channels, color, phase, ccs);
    FGS_LAUNCH_CHECK("k_asm_phasors");
    launch_splat_fwd<true>(p.base, sv, 1u, ccs, field, dw, st);
    FGS_LAUNCH_CHECK("k_wave_splat");
    fgs_stage_end(ST_SPLAT_FWD, st);
    fgs_stage_begin(ST_FIELD_FWD, st);
    float *pmax = reinterpret_cast<float *>(sc + p.c_part);
    hipLaunchKernelGGL(k_wave_max, dim3(RED_BLOCKS, B), dim3(256), 0, st, HW, field, pmax);
    FGS_LAUNCH_CHECK("k_wave_max");
    hipLaunchKernelGGL(k_wave_output, dim3((unsigned)((HW + 255) / 256), B), dim3(256), 0, st, HW, p.w.background[0],
                       p.w.background[1], p.w.background[2], field, dw, pmax, scal, out_rgb, out_depth,
                       reinterpret_cast<const uint32_t *>(sv + p.base.L.seg_off), (uint32_t)p.base.tiles);
    FGS_LAUNCH_CHECK("k_wave_output");
    fgs_stage_end(ST_FIELD_FWD, st);
    return FGS_OK;
}

int fgs_wave_backward(const FgsWaveDims *dims, const float *cameras, const float *pos, const float *scale,
                      const float *quat, const float *color, const float *opacity, const float *phase,
                      void *saved, void *scratch, const float *g_rgb, const float *g_depth, float *g_pos,
                      float *g_scale, float *g_quat, float *g_color, float *g_opacity, float *g_phase,
                      void *stream) {
    WavePlan p;
    int rc = make_wave_plan(dims, &p);
    if (rc) return rc;
    const void *ptrs[] = {cameras, pos, scale, quat, color, opacity, phase, saved, scratch, g_rgb, g_depth,
                          g_pos, g_scale, g_quat, g_color, g_opacity, g_phase};
    if ((rc = check_ptrs(ptrs, 17, "fgs_wave_backward"))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *sv = reinterpret_cast<char *>(saved), *sc = reinterpret_cast<char *>(scratch);
    const int B = p.w.batch;
    const size_t HW = p.HW;
    float2 *field = reinterpret_cast<float2 *>(sv + p.v_field);
    float2 *dw = reinterpret_cast<float2 *>(sv + p.v_dw);
    float *scal = reinterpret_cast<float *>(sv + p.v_scal);
    float2 *gfield = reinterpret_cast<float2 *>(sc + p.c_gfield);
    float2 *gdw = reinterpret_cast<float2 *>(sc + p.c_gdw);
    float *rows = reinterpret_cast<float *>(sc + p.c_rows);
    fgs_stage_begin(ST_FIELD_BWD, st);
    const dim3 gpix((unsigned)((HW + 255) / 256), B);
    float2 *psum = reinterpret_cast<float2 *>(sc + p.c_part);
    hipLaunchKernelGGL(k_wave_output_bwd1, dim3(RED_BLOCKS, B), dim3(256), 0, st, HW, p.w.background[0],
                       p.w.background[1], p.w.background[2], field, scal, g_rgb, psum);
    FGS_LAUNCH_CHECK("k_wave_output_bwd1");
    hipLaunchKernelGGL(k_wave_output_bwd2, gpix, dim3(256), 0, st, HW, p.w.background[0], p.w.background[1],
                       p.w.background[2], field, dw, scal, psum, g_rgb, g_depth, gfield, gdw);
    FGS_LAUNCH_CHECK("k_wave_output_bwd2");
    fgs_stage_end(ST_FIELD_BWD, st);
    fgs_stage_begin(ST_SPLAT_BWD, st);
    launch_splat_bwd<true>(p.base, sv, 1u, reinterpret_cast<const float *>(sv + p.v_ccs), gfield, rows, gdw, st);
    FGS_LAUNCH_CHECK("k_wave_splat_bwd");
    fgs_stage_end(ST_SPLAT_BWD, st);
    fgs_stage_begin(ST_PROJECT_BWD, st);
    if ((rc = fgs_launch_asm_project_bwd(p.base, cameras, pos, scale, quat, color, phase, p.w.phase_channels, sv, rows,
                                         g_pos, g_scale, g_quat, g_color, g_opacity, g_phase, st, true)))
        return rc;
    fgs_stage_end(ST_PROJECT_BWD, st);
    return FGS_OK;
}

}  // extern "C"
