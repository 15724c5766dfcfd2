// deskew_math.h -- the arithmetic of pcr_deskew (include/pcr_hip.h), for device and host: the control table the host prepares from the caller's
// motion, the trajectory evaluated at a time, one point moved from its own time's frame into the reference time's, and -- host only -- the checks
// and the loop of pcr_deskew_host, which is the definition: deskew.hip's kernel runs the same functions and must produce their bits.
// Only f64 + - * /, sqrt (correctly rounded on the host and on gfx950) and conversions, under -ffp-contract=off as in the library: no
// math-library call, no HIP call; a host compiler takes the header as it is (host/deskew_check.cpp).  DESIGN 4.20.
//
// The interpolation is NORMALISED LINEAR interpolation of the unit quaternion (nlerp), not slerp: inside a segment whose two rotations differ
// by theta, the interpolated rotation is off the constant-angular-velocity one by at most theta^3 / 240 rad for theta <= 1 rad (leading term
// theta^3 / 249, at s ~ 0.21 and 0.79; checked numerically on the CPU for theta = 0.01 ... 1 rad: tests/test_deskew_host.py).  That is
// 5.7e-7 rad for 3 degrees and 2.1e-5 rad for 10 degrees in one segment; a caller who wants less supplies denser control poses.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pcr_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSK_HD __host__ __device__ inline
#else
#define DSK_HD inline
#endif

namespace pcr {
namespace dsk {

constexpr size_t kMinK = 2, kMaxK = 1024;
// a control pose's record: the unit quaternion (x, y, z, w), the translation, the stamp
constexpr int kRec = 8, kQ = 0, kP = 4, kTau = 7;

// x - x is 0 for every finite x and NaN for an infinity or a NaN
DSK_HD bool finite1(double x) { return x - x == 0.0; }

DSK_HD int time_bytes(int kind) { return kind == PCR_TIME_F64_SECONDS ? 8 : 4; }

// tau of a time field whose bytes are w0 (and w1, the upper half of a double)
DSK_HD double time_of(int kind, uint32_t w0, uint32_t w1, double t0) {
    if (kind == PCR_TIME_F32_SECONDS) {
        float f;
        __builtin_memcpy(&f, &w0, 4);
        return t0 + (double)f;
    }
    if (kind == PCR_TIME_U32_NANOSECONDS) return t0 + (double)w0 * 1e-9;
    const uint64_t b = (uint64_t)w0 | ((uint64_t)w1 << 32);
    double d;
    __builtin_memcpy(&d, &b, 8);
    return t0 + d;
}

// Record j of the table from control pose T (column-major 4x4) and its stamp: Eigen's Quaternion(Matrix3) as small_math.h's t2se3 restates it,
// normalised; prev (the record before, or nullptr): the sign that makes the four-term dot product with it non-negative.
inline void make_record(const double* T, double stamp, const double* prev, double* rec) {
#define M_(i, j) T[(j) * 4 + (i)]
    double q[4];
    double t = (M_(0, 0) + M_(1, 1)) + M_(2, 2);
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (M_(2, 1) - M_(1, 2)) * t; q[1] = (M_(0, 2) - M_(2, 0)) * t; q[2] = (M_(1, 0) - M_(0, 1)) * t;
    } else {
        int i = 0;
        if (M_(1, 1) > M_(0, 0)) i = 1;
        if (M_(2, 2) > M_(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(((M_(i, i) - M_(j, j)) - M_(k, k)) + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (M_(k, j) - M_(j, k)) * t;
        q[j] = (M_(j, i) + M_(i, j)) * t;
        q[k] = (M_(k, i) + M_(i, k)) * t;
    }
#undef M_
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int c = 0; c < 4; ++c) q[c] = q[c] / n;
    if (prev) {
        const double dot = ((q[0] * prev[0] + q[1] * prev[1]) + q[2] * prev[2]) + q[3] * prev[3];
        if (dot < 0.0) for (int c = 0; c < 4; ++c) q[c] = -q[c];
    }
    for (int c = 0; c < 4; ++c) rec[kQ + c] = q[c];
    rec[kP] = T[12]; rec[kP + 1] = T[13]; rec[kP + 2] = T[14];
    rec[kTau] = stamp;
}

// The trajectory at tau: R (row-major 3x3) and p.  Returns -1 / +1 when tau was clamped to the first / last stamp, else 0.  Reads records
// [0, K) of tab and nothing else: j stays in [0, K - 2].
DSK_HD int eval(const double* tab, int K, double tau, double* R, double* p) {
    int clamped = 0;
    const double t_lo = tab[kTau], t_hi = tab[(size_t)(K - 1) * kRec + kTau];
    if (tau < t_lo) { tau = t_lo; clamped = -1; }
    else if (tau > t_hi) { tau = t_hi; clamped = 1; }
    int lo = 0, hi = K - 2;      // the largest j of [0, K - 2] with tau_j <= tau
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[(size_t)mid * kRec + kTau] <= tau) lo = mid; else hi = mid - 1;
    }
    const double* a = tab + (size_t)lo * kRec;
    const double* b = a + kRec;
    const double s = (tau - a[kTau]) / (b[kTau] - a[kTau]);
    const double u = 1.0 - s;
    const double q0 = u * a[0] + s * b[0], q1 = u * a[1] + s * b[1], q2 = u * a[2] + s * b[2], q3 = u * a[3] + s * b[3];
    p[0] = u * a[kP] + s * b[kP]; p[1] = u * a[kP + 1] + s * b[kP + 1]; p[2] = u * a[kP + 2] + s * b[kP + 2];
    const double n = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const double x = q0 / n, y = q1 / n, z = q2 / n, w = q3 / n;
    // Eigen's toRotationMatrix, as t2se3 closes
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
    return clamped;
}

// One point: from the sensor frame at its own time (R, p) into the sensor frame at the reference time (Rr, pr), rounded to float
DSK_HD void move_point(const double* R, const double* p, const double* Rr, const double* pr, float fx, float fy, float fz, float* o) {
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    const double d0 = (((R[0] * x + R[1] * y) + R[2] * z) + p[0]) - pr[0];
    const double d1 = (((R[3] * x + R[4] * y) + R[5] * z) + p[1]) - pr[1];
    const double d2 = (((R[6] * x + R[7] * y) + R[8] * z) + p[2]) - pr[2];
    o[0] = (float)((Rr[0] * d0 + Rr[3] * d1) + Rr[6] * d2);
    o[1] = (float)((Rr[1] * d0 + Rr[4] * d1) + Rr[7] * d2);
    o[2] = (float)((Rr[2] * d0 + Rr[5] * d1) + Rr[8] * d2);
}

// A record is moved when its coordinates and its tau are finite; otherwise it is copied unchanged and counted
DSK_HD bool record_finite(float fx, float fy, float fz, double tau) {
    return finite1((double)fx) && finite1((double)fy) && finite1((double)fz) && finite1(tau);
}

// ---- host only (plain host functions: a device pass parses them and emits nothing): the checks both entry points make, the preparation, and pcr_deskew_host's loop ----

struct Call {
    const void* pts; size_t n, stride; const void* times; int kind; long long off; const pcr_deskew_motion* m; void* out;
    bool same_space;      // pts (with times) and out live in one memory space: their ranges can be compared
};

// the reference pose of a prepared motion
struct Ref { double R[9], p[3]; int clamped; };

// Why the call is refused, naming the field; nullptr when it is in order.  On success tab holds m->K records (kRec * kMaxK doubles of room) and
// ref the trajectory at t_ref.  Nothing of the caller's is written.
inline const char* prepare(const Call& c, double* tab, Ref* ref) {
    if (c.stride < 16 || c.stride % 4 != 0) return "stride_bytes must be a multiple of 4 and >= 16";
    if (c.kind != PCR_TIME_F32_SECONDS && c.kind != PCR_TIME_U32_NANOSECONDS && c.kind != PCR_TIME_F64_SECONDS)
        return "time_kind must be PCR_TIME_F32_SECONDS, PCR_TIME_U32_NANOSECONDS or PCR_TIME_F64_SECONDS";
    const size_t eb = (size_t)time_bytes(c.kind);
    if (!c.times) {
        if (c.off < 12) return "time_offset_bytes lies in the coordinates (or is negative)";
        if ((size_t)c.off % eb != 0) return "time_offset_bytes must be a multiple of the time element's size";
        if ((size_t)c.off > c.stride || c.stride - (size_t)c.off < eb) return "time_offset_bytes: the time field must lie inside stride_bytes";
    }
    if (c.n > SIZE_MAX / c.stride) return "n * stride_bytes overflows";
    if (c.n && !c.pts) return "pts is NULL";
    if (c.n && !c.out) return "out is NULL";
    const pcr_deskew_motion* m = c.m;
    if (!m) return "the motion m is NULL";
    if (m->K < kMinK || m->K > kMaxK) return "m->K must be 2..1024";
    if (!m->poses) return "m->poses is NULL";
    if (!m->stamps) return "m->stamps is NULL";
    if (!finite1(m->t0)) return "m->t0 is not finite";
    if (!finite1(m->t_ref)) return "m->t_ref is not finite";
    for (size_t j = 0; j < m->K; ++j) {
        if (!finite1(m->stamps[j])) return "m->stamps holds a value that is not finite";
        if (j && !(m->stamps[j] > m->stamps[j - 1])) return "m->stamps must be strictly increasing";
    }
    for (size_t i = 0; i < 16 * m->K; ++i) if (!finite1(m->poses[i])) return "m->poses holds a value that is not finite";
    if (c.n && c.same_space) {
        const char* a = (const char*)c.pts;
        const char* o = (const char*)c.out;
        const size_t bytes = c.n * c.stride;
        if (o != a && o < a + bytes && a < o + bytes) return "out overlaps pts without being pts (in place: out == pts)";
        if (c.times) {
            const char* t = (const char*)c.times;
            if (o < t + c.n * eb && t < o + bytes) return "out overlaps times";
        }
    }
    for (size_t j = 0; j < m->K; ++j) {
        make_record(m->poses + 16 * j, m->stamps[j], j ? tab + (j - 1) * kRec : nullptr, tab + j * kRec);
        for (int k = 0; k < 4; ++k) if (!finite1(tab[j * kRec + k])) return "m->poses holds a rotation that yields no finite unit quaternion";
    }
    ref->clamped = eval(tab, (int)m->K, m->t_ref, ref->R, ref->p) != 0;
    return nullptr;
}

// the 4-byte words of a record's (or the packed array's) time field, read without an alignment assumption
inline void time_words(const Call& c, size_t i, uint32_t* w0, uint32_t* w1) {
    const char* src = c.times ? (const char*)c.times + i * (size_t)time_bytes(c.kind) : (const char*)c.pts + i * c.stride + (size_t)c.off;
    *w1 = 0;
    memcpy(w0, src, 4);
    if (c.kind == PCR_TIME_F64_SECONDS) memcpy(w1, src + 4, 4);
}

// pcr_deskew_host without its error channel: nullptr, or the refusal.  info may be nullptr.
inline const char* deskew_host(const Call& c, pcr_deskew_info* info) {
    static_assert(kRec * sizeof(double) == 64, "a record is 64 bytes");
    double tab[kRec * kMaxK];
    Ref ref;
    if (const char* why = prepare(c, tab, &ref)) return why;
    pcr_deskew_info inf;
    memset(&inf, 0, sizeof inf);
    inf.ref_clamped = ref.clamped;
    const int K = (int)c.m->K;
    for (size_t i = 0; i < c.n; ++i) {
        const char* rec = (const char*)c.pts + i * c.stride;
        char* dst = (char*)c.out + i * c.stride;
        uint32_t w0, w1;
        time_words(c, i, &w0, &w1);      // (before the record is written: in place, the time may be a field of it)
        float f[3];
        memcpy(f, rec, 12);
        if (dst != rec) memmove(dst, rec, c.stride);
        const double tau = time_of(c.kind, w0, w1, c.m->t0);
        if (!record_finite(f[0], f[1], f[2], tau)) { inf.nonfinite += 1; continue; }
        double R[9], p[3];
        const int cl = eval(tab, K, tau, R, p);
        inf.before += cl < 0; inf.after += cl > 0;
        float o[3];
        move_point(R, p, ref.R, ref.p, f[0], f[1], f[2], o);
        memcpy(dst, o, 12);
    }
    if (info) *info = inf;
    return nullptr;
}

}  // namespace dsk
}  // namespace pcr
