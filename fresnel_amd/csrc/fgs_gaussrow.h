// Pieces shared by the per-Gaussian elementwise units (fgs_head.hip, fgs_saag.hip): whole-tile copies between global memory and
// LDS for rows of odd width, and rotation_6d_to_quaternion (GDM:186-276) with its adjoint.  Everything sits in an anonymous
// namespace: each unit compiles its own copy under its own flags (-ffp-contract=off in both, fresnel_amd/build.py), and a unit
// that recomputes the forward in its backward gets the forward's roundings.
#ifndef FGS_GAUSSROW_H
#define FGS_GAUSSROW_H

#include "fgs_internal.h"

namespace {

constexpr int HB = 256;         // threads per block, and the most rows of a tile
constexpr float EPS = 1e-6f;    // F.normalize(eps=1e-6) and the b3 fallback threshold

// ---- tile copies ----------------------------------------------------------------------------------------------------------------
// n floats, global -> dense LDS (16-byte aligned)
__device__ __forceinline__ void tile_load(float *lds, const float *src, int n, int tid) {
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += HB) reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(src)[i];
        done = n4 << 2;
    }
    for (int e = done + tid; e < n; e += HB) lds[e] = src[e];
}

// n floats, dense LDS (16-byte aligned) -> global
__device__ __forceinline__ void tile_store(float *dst, const float *lds, int n, int tid) {
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += HB) reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(lds)[i];
        done = n4 << 2;
    }
    for (int e = done + tid; e < n; e += HB) dst[e] = lds[e];
}

// rows of C floats: global (dense) <-> LDS at the odd row stride CP
template <int C, int CP>
__device__ __forceinline__ int padded(int e) {
    const int row = e / C;
    return row * CP + (e - row * C);
}

template <int C, int CP>
__device__ __forceinline__ void rows_load(float *lds, const float *src, int nrows, int tid) {
    const int n = nrows * C;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += HB) {
            const float4 v = reinterpret_cast<const float4 *>(src)[i];
            const int e = i << 2;
            lds[padded<C, CP>(e)] = v.x; lds[padded<C, CP>(e + 1)] = v.y;
            lds[padded<C, CP>(e + 2)] = v.z; lds[padded<C, CP>(e + 3)] = v.w;
        }
        done = n4 << 2;
    }
    for (int e = done + tid; e < n; e += HB) lds[padded<C, CP>(e)] = src[e];
}

template <int C, int CP>
__device__ __forceinline__ void rows_store(float *dst, const float *lds, int nrows, int tid) {
    const int n = nrows * C;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += HB) {
            const int e = i << 2;
            reinterpret_cast<float4 *>(dst)[i] = make_float4(lds[padded<C, CP>(e)], lds[padded<C, CP>(e + 1)],
                                                             lds[padded<C, CP>(e + 2)], lds[padded<C, CP>(e + 3)]);
        }
        done = n4 << 2;
    }
    for (int e = done + tid; e < n; e += HB) dst[e] = lds[padded<C, CP>(e)];
}

// ---- small vectors --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const float *a, const float *b, float *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// adjoint of y = v / max(|v|, eps) (F.normalize): through the norm where it is not clamped (closed interval, as torch's clamp_min)
template <int N>
__device__ __forceinline__ void normalize_bwd(const float *v, float n, const float *g, float *gv) {
    if (n >= EPS) {
        float gdotv = 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) gdotv += g[i] * v[i];
        const float w = gdotv / (n * n * n);
#pragma unroll
        for (int i = 0; i < N; ++i) gv[i] = g[i] / n - v[i] * w;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) gv[i] = g[i] / EPS;
    }
}

// ---- rotation_6d_to_quaternion (GDM:186-276) with +1e-8 in place of the reference's random sign -----------
struct Rot {
    float n1, b1[3], d, v2[3], n2, b2[3], sel[3], m3, b3[3], t, s, qr[4], nq;
    int branch;
    bool replaced;
};

__device__ __forceinline__ void rot_fwd(const float *a1, const float *a2, Rot &r, float *q) {
    r.n1 = sqrtf(dot3(a1, a1));
    const float den1 = fmaxf(r.n1, EPS);
#pragma unroll
    for (int i = 0; i < 3; ++i) r.b1[i] = a1[i] / den1;
    r.d = dot3(r.b1, a2);
#pragma unroll
    for (int i = 0; i < 3; ++i) r.v2[i] = a2[i] - r.d * r.b1[i] + 1e-8f;
    r.n2 = sqrtf(dot3(r.v2, r.v2));
    const float den2 = fmaxf(r.n2, EPS);
#pragma unroll
    for (int i = 0; i < 3; ++i) r.b2[i] = r.v2[i] / den2;
    cross3(r.b1, r.b2, r.sel);
    r.replaced = sqrtf(dot3(r.sel, r.sel)) < EPS;
    if (r.replaced) { r.sel[0] = 0.0f; r.sel[1] = 0.0f; r.sel[2] = 1.0f; }
    r.m3 = sqrtf(dot3(r.sel, r.sel));
    const float den3 = fmaxf(r.m3, EPS);
#pragma unroll
    for (int i = 0; i < 3; ++i) r.b3[i] = r.sel[i] / den3;
    // R = [b1 b2 b3] (columns): Rij = b_{j+1}[i]
    const float R00 = r.b1[0], R01 = r.b2[0], R02 = r.b3[0];
    const float R10 = r.b1[1], R11 = r.b2[1], R12 = r.b3[1];
    const float R20 = r.b1[2], R21 = r.b2[2], R22 = r.b3[2];
    const float trace = R00 + R11 + R22;
    if (trace > 0.0f) {
        r.branch = 0; r.t = trace + 1.0f;
    } else if (R00 > R11 && R00 > R22) {
        r.branch = 1; r.t = 1.0f + R00 - R11 - R22;
    } else if (R11 > R22) {
        r.branch = 2; r.t = 1.0f + R11 - R00 - R22;
    } else {
        r.branch = 3; r.t = 1.0f + R22 - R00 - R11;
    }
    r.s = sqrtf(fmaxf(r.t, 1e-10f)) * 2.0f;
    const float big = 0.25f * r.s;
    switch (r.branch) {
    case 0: r.qr[0] = big; r.qr[1] = (R21 - R12) / r.s; r.qr[2] = (R02 - R20) / r.s; r.qr[3] = (R10 - R01) / r.s; break;
    case 1: r.qr[0] = (R21 - R12) / r.s; r.qr[1] = big; r.qr[2] = (R01 + R10) / r.s; r.qr[3] = (R02 + R20) / r.s; break;
    case 2: r.qr[0] = (R02 - R20) / r.s; r.qr[1] = (R01 + R10) / r.s; r.qr[2] = big; r.qr[3] = (R12 + R21) / r.s; break;
    default: r.qr[0] = (R10 - R01) / r.s; r.qr[1] = (R02 + R20) / r.s; r.qr[2] = (R12 + R21) / r.s; r.qr[3] = big; break;
    }
    r.nq = sqrtf(r.qr[0] * r.qr[0] + r.qr[1] * r.qr[1] + r.qr[2] * r.qr[2] + r.qr[3] * r.qr[3]);
    const float denq = fmaxf(r.nq, EPS);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = r.qr[i] / denq;
}

// adjoint of rot_fwd: only the selected branch is differentiated
__device__ __forceinline__ void rot_bwd(const float *a1, const float *a2, const Rot &r, const float *gq, float *ga1, float *ga2) {
    float gqr[4];
    normalize_bwd<4>(r.qr, r.nq, gq, gqr);
    // gR[i][j] = dL/dRij; every off-diagonal quotient is (Rab -+ Rba) / s, the branch's own component is s / 4
    float gR[3][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    const float is = 1.0f / r.s;
    float gs = 0.0f;
    auto quot = [&](int comp, int a, int b, int c, int d, float sign) {  // q[comp] = (R[a][b] + sign R[c][d]) / s
        const float g = gqr[comp] * is;
        gR[a][b] += g;
        gR[c][d] += sign * g;
        gs -= gqr[comp] * r.qr[comp] * is;
    };
    float sg[3];
    switch (r.branch) {
    case 0:
        gs += 0.25f * gqr[0];
        quot(1, 2, 1, 1, 2, -1.0f); quot(2, 0, 2, 2, 0, -1.0f); quot(3, 1, 0, 0, 1, -1.0f);
        sg[0] = 1.0f; sg[1] = 1.0f; sg[2] = 1.0f;
        break;
    case 1:
        gs += 0.25f * gqr[1];
        quot(0, 2, 1, 1, 2, -1.0f); quot(2, 0, 1, 1, 0, 1.0f); quot(3, 0, 2, 2, 0, 1.0f);
        sg[0] = 1.0f; sg[1] = -1.0f; sg[2] = -1.0f;
        break;
    case 2:
        gs += 0.25f * gqr[2];
        quot(0, 0, 2, 2, 0, -1.0f); quot(1, 0, 1, 1, 0, 1.0f); quot(3, 1, 2, 2, 1, 1.0f);
        sg[0] = -1.0f; sg[1] = 1.0f; sg[2] = -1.0f;
        break;
    default:
        gs += 0.25f * gqr[3];
        quot(0, 1, 0, 0, 1, -1.0f); quot(1, 0, 2, 2, 0, 1.0f); quot(2, 1, 2, 2, 1, 1.0f);
        sg[0] = -1.0f; sg[1] = -1.0f; sg[2] = 1.0f;
        break;
    }
    const float gt = r.t >= 1e-10f ? gs * 2.0f * is : 0.0f;  // s = 2 sqrt(t): ds/dt = 2 / s
#pragma unroll
    for (int i = 0; i < 3; ++i) gR[i][i] += sg[i] * gt;
    float gb1[3], gb2[3], gb3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { gb1[i] = gR[i][0]; gb2[i] = gR[i][1]; gb3[i] = gR[i][2]; }
    if (!r.replaced) {  // b3 = normalize(b1 x b2); the (0, 0, 1) fallback is a constant
        float gsel[3], c[3];
        normalize_bwd<3>(r.sel, r.m3, gb3, gsel);
        cross3(r.b2, gsel, c);
#pragma unroll
        for (int i = 0; i < 3; ++i) gb1[i] += c[i];
        cross3(gsel, r.b1, c);
#pragma unroll
        for (int i = 0; i < 3; ++i) gb2[i] += c[i];
    }
    float gv2[3];
    normalize_bwd<3>(r.v2, r.n2, gb2, gv2);
    const float gd = -dot3(gv2, r.b1);  // v2 = a2 - d b1 + 1e-8, d = b1 . a2
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ga2[i] = gv2[i] + gd * r.b1[i];
        gb1[i] += gd * a2[i] - r.d * gv2[i];
    }
    normalize_bwd<3>(a1, r.n1, gb1, ga1);
}

}  // namespace

#endif  // FGS_GAUSSROW_H
