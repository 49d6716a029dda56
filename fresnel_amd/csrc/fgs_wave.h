// Wave64 cross-lane reductions and list-staging helpers for gfx950, shared by the composite and ASM kernels.
#pragma once

// Staging-time decode (per lane, parallel over the chunk) of a record's bbox against the tile of NSX x 2 sub-tiles (8x8 each; 16 or 32
// pixels wide) at (X0, Y0) -- the ONE decoder of the blend kernels (k_composite_fwd, k_blend_fwd_parts, k_composite_bwd) and of the
// splat (k_asm_splat, which passes opacity 1 and uses the touched bits and the pixel bits only):
//   flags  bits 0 .. 2 NSX - 1: sub-tile s = row * NSX + col intersects the bbox [x0, x1) x [y0, y1) -- all clear when the opacity is
//                 negative (alpha clamps to 0 with zero gradient, DR:646: the record contributes nothing);
//          bit 8: the alpha clamp cannot bind (opacity <= 0.98 and `conic_ok`, the caller's check that the quadratic form is positive
//                 definite with a margin): G op / 0.99 = exp2(m' + log2(opacity / 0.99)), as the blend kernels form it (the opacity
//                 folded into the exponent, fgs_internal.h), stays below 1 whatever the pixel, so the clamp modifier of the v_exp is
//                 idle and the backward needs no clamp-gradient select.  For a regularised inverse covariance that came out
//                 indefinite in fp32 (needles, edge-on discs) G can exceed 1.0102 and the clamp of DR:647 does bind -- those keep
//                 the clamped path;
//          bits 16-31: pixel row Y0 + i lies in [y0, y1);
//   cbits  bit i (i < 8 NSX): pixel column X0 + i lies in [x0, x1).
// In the list loop a lane turns its column / row bit into an all-ones / zero mask with one v_bfe_i32.
template <int NSX>
__device__ __forceinline__ void stage_decode_w(uint32_t X0, uint32_t Y0, uint32_t bbx, uint32_t bby, float op,
                                               uint32_t &flags, uint32_t &cbits, bool conic_ok = true) {
    constexpr int TW = 8 * NSX;
    const int x0 = (int)(bbx & 0xFFFFu), x1 = (int)(bbx >> 16), y0 = (int)(bby & 0xFFFFu), y1 = (int)(bby >> 16);
    const int lx0 = max(x0 - (int)X0, 0), lx1 = min(x1 - (int)X0, TW);
    const int ly0 = max(y0 - (int)Y0, 0), ly1 = min(y1 - (int)Y0, 16);
    cbits = lx1 > lx0 ? (uint32_t)(((1ull << (lx1 - lx0)) - 1ull) << lx0) : 0u;
    const uint32_t ym = ly1 > ly0 ? ((1u << (ly1 - ly0)) - 1u) << ly0 : 0u;
    uint32_t touched = 0;
    if (op >= 0.0f) {
#pragma unroll
        for (int c = 0; c < NSX; ++c) {
            const uint32_t cm = (cbits >> (8 * c)) & 0xFFu;
            if (cm && (ym & 0xFFu)) touched |= 1u << c;
            if (cm && (ym >> 8)) touched |= 1u << (NSX + c);
        }
    }
    flags = touched | ((op <= 0.98f && conic_ok) ? 256u : 0u) | (ym << 16);
}

// (x < lim) ? v : 0.  The compare and the select are kept ADJACENT in one asm block: a v_cndmask reading VCC
// straight after the v_cmp that wrote it issues in ~2.6 cycles on gfx950, any other VCC-reading v_cndmask in
// 14-23 (scratch/ubench/valu3.hip, valu4.hip).
__device__ __forceinline__ float select_lt(float x, float lim, float v) {
    float o;
    asm("v_cmp_lt_f32 vcc, %1, %2\n\tv_cndmask_b32 %0, 0, %3, vcc" : "=v"(o) : "v"(x), "v"(lim), "v"(v) : "vcc");
    return o;
}

// (a == b) ? v : 0, compare and select adjacent (see select_lt)
__device__ __forceinline__ float select_eq(float a, float b, float v) {
    float o;
    asm("v_cmp_eq_f32 vcc, %1, %2\n\tv_cndmask_b32 %0, 0, %3, vcc" : "=v"(o) : "v"(a), "v"(b), "v"(v) : "vcc");
    return o;
}
// x >= lim ? (a, b) : (c, 0): ONE compare, both selects right behind it
__device__ __forceinline__ void select2_ge(float x, float lim, float a, float b, float c, float &o1, float &o2) {
    asm("v_cmp_ge_f32 vcc, %2, %3\n\tv_cndmask_b32 %0, %6, %4, vcc\n\tv_cndmask_b32 %1, 0, %5, vcc"
        : "=&v"(o1), "=&v"(o2) : "v"(x), "v"(lim), "v"(a), "v"(b), "v"(c) : "vcc");
}

// Quad sum of one value: lanes with (lane & 3) == 3 end up with the sum over their quad.
__device__ __forceinline__ void quad_sum1(float &a) {
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
                 "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n" : "+v"(a));
}

// Sum NV per-lane values over the 64 lanes of a wave through LDS, transposed (NV <= 16): every lane parks its NV
// partial sums; lane 4 k + p then adds the 16 partials of part p of value k (four ds_read_b128, 15 adds) and two DPP
// steps fold the four parts -- ~NV LDS stores + 15 plain adds + 2 DPP adds per call, against NV x 6 DPP adds (4.3 issue
// cycles each on gfx950) for a full DPP tree.  One wave's LDS instructions execute in order, so no barrier is needed;
// the scratch is private to the calling wave.
// ---- parking with ds_write_addtid_b32 ----------------------------------------------------------------------------
// Layout: value k at dword 68 k, lane l's partial at 68 k + l (ds_write_addtid_b32: address = M0 + offset + 4 lane,
// no address VGPR, 2 store-path cycles per instruction instead of 4-6, MI355X_MICROARCH.md "LDS").  Lane 4 k + p then
// reads the 16 partials [16 p, 16 p + 16) of value k with four ds_read_b128; with the 68-dword pitch the 16 lanes of
// every ds_read_b128 group touch 16 different 4-bank slots (banks 4 k + 16 p + m mod 64), so both sides are
// conflict-free (the [80]-pitch layout above cost 29 % of the LDS cycles in conflicts).  M0 is saved and restored.
typedef __attribute__((address_space(3))) float fgs_lds_float;
#define FGS_RED_PITCH 68
// Parking of NV = 10 ... 13 values (10: blend backward, 11: phase backward, 12 / 13: ASM / wave splat backward), one overload per NV
// from one macro.  ALL stores of a call and the M0 save / restore sit in ONE asm block: M0 must not be live across
// compiler-scheduled code (every DS instruction reads it).  `red` = FGS_RED_PITCH * NV floats of LDS private to the calling wave.
#define FGS_PARK_ST(k, off) "ds_write_addtid_b32 %[v" #k "] offset:" #off "\n\t"
#define FGS_PARK_OP(k) [v##k] "v"(v[k])
#define FGS_PARK_ST10                                                                                              \
    FGS_PARK_ST(0, 0) FGS_PARK_ST(1, 272) FGS_PARK_ST(2, 544) FGS_PARK_ST(3, 816) FGS_PARK_ST(4, 1088)             \
    FGS_PARK_ST(5, 1360) FGS_PARK_ST(6, 1632) FGS_PARK_ST(7, 1904) FGS_PARK_ST(8, 2176) FGS_PARK_ST(9, 2448)
#define FGS_PARK_OP10                                                                                              \
    FGS_PARK_OP(0), FGS_PARK_OP(1), FGS_PARK_OP(2), FGS_PARK_OP(3), FGS_PARK_OP(4), FGS_PARK_OP(5), FGS_PARK_OP(6), \
    FGS_PARK_OP(7), FGS_PARK_OP(8), FGS_PARK_OP(9)
#define FGS_DEFINE_PARK(NV, STORES, ...)                                                                           \
    __device__ __forceinline__ void addtid_park(float *red, const float (&v)[NV]) {                                \
        uint32_t m0_save;                                                                                          \
        asm volatile("s_mov_b32 %[save], m0\n\ts_mov_b32 m0, %[base]\n\ts_nop 0\n\t" STORES "s_mov_b32 m0, %[save]"  \
                     : [save] "=&s"(m0_save)                                                                       \
                     : __VA_ARGS__, [base] "s"((uint32_t)(uintptr_t)(fgs_lds_float *)red)                          \
                     : "memory");                                                                                  \
    }
// (6: one dead-unit entry of the blend backward, which parks two entries' values side by side: cells 0-5 and 6-11 of one `red`)
FGS_DEFINE_PARK(6, FGS_PARK_ST(0, 0) FGS_PARK_ST(1, 272) FGS_PARK_ST(2, 544) FGS_PARK_ST(3, 816) FGS_PARK_ST(4, 1088) FGS_PARK_ST(5, 1360),
                FGS_PARK_OP(0), FGS_PARK_OP(1), FGS_PARK_OP(2), FGS_PARK_OP(3), FGS_PARK_OP(4), FGS_PARK_OP(5))
FGS_DEFINE_PARK(10, FGS_PARK_ST10, FGS_PARK_OP10)
FGS_DEFINE_PARK(11, FGS_PARK_ST10 FGS_PARK_ST(10, 2720), FGS_PARK_OP10, FGS_PARK_OP(10))
FGS_DEFINE_PARK(12, FGS_PARK_ST10 FGS_PARK_ST(10, 2720) FGS_PARK_ST(11, 2992), FGS_PARK_OP10, FGS_PARK_OP(10), FGS_PARK_OP(11))
FGS_DEFINE_PARK(13, FGS_PARK_ST10 FGS_PARK_ST(10, 2720) FGS_PARK_ST(11, 2992) FGS_PARK_ST(12, 3264), FGS_PARK_OP10, FGS_PARK_OP(10),
                FGS_PARK_OP(11), FGS_PARK_OP(12))
#undef FGS_DEFINE_PARK
#undef FGS_PARK_OP10
#undef FGS_PARK_ST10
#undef FGS_PARK_OP
#undef FGS_PARK_ST

// Second half of the sum: adds the parked values up; returns, in lanes with (lane & 3) == 3 and lane < 4 nv, the total of value
// lane >> 2 (other lanes below 4 nv: junk; lanes >= 4 nv: +0.0f, which the blend backward's dead walk stores).  `red` is 16-B aligned.
__device__ __forceinline__ float wave_sum_addtid_finish(const float *red, uint32_t lane, uint32_t nv) {
    __builtin_amdgcn_wave_barrier();
    float tot = 0.0f;
    if (lane < 4u * nv) {
        const float4 *src = reinterpret_cast<const float4 *>(red + FGS_RED_PITCH * (lane >> 2) + 16u * (lane & 3u));
        const float4 s0 = src[0], s1 = src[1], s2 = src[2], s3 = src[3];
        tot = ((s0.x + s0.y) + (s0.z + s0.w)) + ((s1.x + s1.y) + (s1.z + s1.w)) +
              (((s2.x + s2.y) + (s2.z + s2.w)) + ((s3.x + s3.y) + (s3.z + s3.w)));
        quad_sum1(tot);
    }
    __builtin_amdgcn_wave_barrier();
    return tot;
}
// Sum NV per-lane values over the wave: park and finish in one call (the blend backward calls the two halves an entry apart)
template <int NV>
__device__ __forceinline__ float wave_sum_addtid(float *red, const float (&v)[NV], uint32_t lane) {
    addtid_park(red, v);
    return wave_sum_addtid_finish(red, lane, (uint32_t)NV);
}
