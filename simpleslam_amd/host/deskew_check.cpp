// deskew_check.cpp -- pcr_deskew_host's body (csrc/deskew_math.h: dsk::deskew_host, which the library's entry point wraps) on the CPU, with no GPU
// call, no HIP header and no library:
//   deskew_check --self
// runs it against hand-worked cases -- a translation, quarter and half turns whose interpolated poses are known in closed form, the sign rule
// of consecutive quaternions, the three time kinds, packed and embedded times, in place and out of place, the clamps, records that are not
// finite, and the refusals (which must leave the output untouched) -- prints one line per case and exits 0 when all pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../csrc/deskew_math.h"

using namespace pcr;

static int g_failed = 0;

static void report(const char* name, bool ok, const std::string& detail = "") {
    printf("%-34s %s%s%s\n", name, ok ? "ok" : "FAILED", detail.empty() ? "" : ": ", detail.c_str());
    if (!ok) ++g_failed;
}

static void rot_z(double deg, double* T) {
    const double a = deg * 3.14159265358979323846 / 180.0;
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    T[0] = cos(a); T[1] = sin(a); T[4] = -sin(a); T[5] = cos(a);      // column-major
}
static void rot_x(double deg, double* T) {
    const double a = deg * 3.14159265358979323846 / 180.0;
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    T[5] = cos(a); T[6] = sin(a); T[9] = -sin(a); T[10] = cos(a);
}

struct Motion {
    std::vector<double> poses, stamps;
    pcr_deskew_motion m{};
    void add(const double* T, double stamp) { poses.insert(poses.end(), T, T + 16); stamps.push_back(stamp); }
    const pcr_deskew_motion* get(double t0, double t_ref) {
        m.poses = poses.data(); m.stamps = stamps.data(); m.K = stamps.size(); m.t0 = t0; m.t_ref = t_ref;
        return &m;
    }
};

static bool near3(const float* p, double x, double y, double z, double tol = 1e-6) {
    return fabs(p[0] - x) <= tol && fabs(p[1] - y) <= tol && fabs(p[2] - z) <= tol;
}

// n points of 4 floats with packed float times -> the output and the counts
static const char* run4(const std::vector<float>& in, const std::vector<float>& times, const pcr_deskew_motion* m, std::vector<float>* out, pcr_deskew_info* info) {
    out->assign(in.size(), -77.0f);
    const dsk::Call c{in.data(), in.size() / 4, 16, times.data(), PCR_TIME_F32_SECONDS, 0, m, out->data(), true};
    return dsk::deskew_host(c, info);
}

static int self_check() {
    double I[16], T[16];
    rot_z(0, I);
    pcr_deskew_info info;
    std::vector<float> out;

    {   // an all-identity motion returns the input bit for bit
        Motion mo; mo.add(I, 0.0); mo.add(I, 1.0);
        const std::vector<float> in = {1.25f, -2.5f, 3.0f, 9.0f, 1e-3f, 63.99f, -17.1f, 8.0f};
        const char* why = run4(in, {0.25f, 0.75f}, mo.get(0.0, 0.5), &out, &info);
        report("identity", !why && memcmp(in.data(), out.data(), in.size() * 4) == 0 && !info.before && !info.after && !info.nonfinite && !info.ref_clamped);
    }
    {   // a translation of 1 m along x over 1 s; t_ref at the start.  Times: inside, on the last stamp, before, after
        Motion mo; mo.add(I, 0.0);
        memcpy(T, I, sizeof T); T[12] = 1.0; mo.add(T, 1.0);
        const std::vector<float> in = {1, 2, 3, 5, 1, 2, 3, 6, 1, 2, 3, 7, 1, 2, 3, 8};
        const char* why = run4(in, {0.5f, 1.0f, -1.0f, 2.0f}, mo.get(0.0, 0.0), &out, &info);
        bool ok = !why && near3(&out[0], 1.5, 2, 3, 0) && near3(&out[4], 2, 2, 3, 0) && near3(&out[8], 1, 2, 3, 0) && near3(&out[12], 2, 2, 3, 0);
        ok = ok && out[3] == 5 && out[7] == 6 && out[11] == 7 && out[15] == 8 && info.before == 1 && info.after == 1 && info.nonfinite == 0 && info.ref_clamped == 0;
        report("translation, clamps", ok);
        // t_ref beyond the range is clamped to the end: the point taken at the end stays where it is
        why = run4(in, {1.0f, 1.0f, 1.0f, 1.0f}, mo.get(0.0, 5.0), &out, &info);
        report("t_ref clamped", !why && info.ref_clamped == 1 && near3(&out[0], 1, 2, 3, 0));
        // t0 shifts every time
        why = run4(in, {0.5f, 0.5f, 0.5f, 0.5f}, mo.get(0.25, 0.0), &out, &info);
        report("t0", !why && near3(&out[0], 1.75, 2, 3, 0));
    }
    {   // a quarter turn about z over 1 s: halfway the interpolation is exactly the eighth turn (symmetry)
        Motion mo; mo.add(I, 0.0); rot_z(90, T); mo.add(T, 1.0);
        const std::vector<float> in = {1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 2, 0};
        const char* why = run4(in, {1.0f, 0.5f, 0.5f}, mo.get(0.0, 0.0), &out, &info);
        const double h = sqrt(0.5);
        report("quarter turn about z", !why && near3(&out[0], 0, 1, 0) && near3(&out[4], h, h, 0) && near3(&out[8], 0, 0, 2));
        why = run4(in, {1.0f, 0.0f, 1.0f}, mo.get(0.0, 1.0), &out, &info);      // t_ref at the end: a point taken then stays, one taken at the start turns back
        report("t_ref at the end", !why && near3(&out[0], 1, 0, 0) && near3(&out[4], 0, -1, 0) && near3(&out[8], 0, 0, 2));
    }
    {   // a half turn about x: trace -1, the quaternion comes from the largest diagonal element; halfway is the quarter turn
        Motion mo; mo.add(I, 0.0); rot_x(180, T); mo.add(T, 1.0);
        const std::vector<float> in = {0, 1, 0, 0, 0, 1, 0, 0};
        const char* why = run4(in, {0.5f, 1.0f}, mo.get(0.0, 0.0), &out, &info);
        report("half turn about x", !why && near3(&out[0], 0, 0, 1) && near3(&out[4], 0, -1, 0));
    }
    {   // Rz(-125) and Rz(-115): the extracted quaternions are (0, 0, +, -) and (0, 0, -, +), their dot product is negative.  With the sign rule the
        // midpoint is Rz(-120); seen from the first pose that is a turn by +5 degrees
        Motion mo; rot_z(-125, T); mo.add(T, 0.0); rot_z(-115, T); mo.add(T, 1.0); rot_z(-105, T); mo.add(T, 2.0);
        double r0[dsk::kRec], r1[dsk::kRec];
        dsk::make_record(&mo.poses[0], 0.0, nullptr, r0);
        dsk::make_record(&mo.poses[16], 1.0, nullptr, r1);
        const bool negative = r0[0] * r1[0] + r0[1] * r1[1] + r0[2] * r1[2] + r0[3] * r1[3] < 0;
        const std::vector<float> in = {1, 0, 0, 0, 1, 0, 0, 0};
        const char* why = run4(in, {0.5f, 1.5f}, mo.get(0.0, 0.0), &out, &info);
        const double d = 3.14159265358979323846 / 180.0;
        report("sign of consecutive quaternions", !why && negative && near3(&out[0], cos(5 * d), sin(5 * d), 0) && near3(&out[4], cos(15 * d), sin(15 * d), 0));
    }
    {   // 32-byte records with the time as a float at byte 24, in place; one NaN coordinate, one NaN time
        Motion mo; mo.add(I, 0.0); memcpy(T, I, sizeof T); T[13] = 2.0; mo.add(T, 1.0);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        std::vector<float> rec = {1, 1, 1, 1, 7, 0, 0.5f, 3,   nan, 1, 1, 1, 7, 0, 0.5f, 3,   1, 1, 1, 1, 7, 0, nan, 3,   2, 2, 2, 1, 8, 0, 0.25f, 4};
        const std::vector<float> before = rec;
        const dsk::Call c{rec.data(), 4, 32, nullptr, PCR_TIME_F32_SECONDS, 24, mo.get(0.0, 0.0), rec.data(), true};
        const char* why = dsk::deskew_host(c, &info);
        bool ok = !why && near3(&rec[0], 1, 2, 1, 0) && near3(&rec[24], 2, 2.5, 2, 0) && info.nonfinite == 2;
        ok = ok && memcmp(&rec[8], &before[8], 64) == 0 && memcmp(&rec[3], &before[3], 20) == 0 && memcmp(&rec[27], &before[27], 20) == 0;
        report("embedded time, in place, NaN", ok);
    }
    {   // nanoseconds and double seconds, packed
        Motion mo; mo.add(I, 0.0); memcpy(T, I, sizeof T); T[14] = 4.0; mo.add(T, 1.0);
        const std::vector<float> in = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t ns[2] = {250000000u, 1000000000u};
        out.assign(8, -77.0f);
        dsk::Call c{in.data(), 2, 16, ns, PCR_TIME_U32_NANOSECONDS, 0, mo.get(0.0, 0.0), out.data(), true};
        const char* why = dsk::deskew_host(c, &info);
        bool ok = !why && near3(&out[0], 0, 0, 1, 0) && near3(&out[4], 0, 0, 4, 0);
        const double sec[2] = {0.75, -3.0};
        c.times = sec; c.kind = PCR_TIME_F64_SECONDS;
        why = dsk::deskew_host(c, &info);
        ok = ok && !why && near3(&out[0], 0, 0, 3, 0) && near3(&out[4], 0, 0, 0, 0) && info.before == 1;
        report("nanoseconds, double seconds", ok);
    }
    {   // the refusals: a reason that names the field, the output untouched
        Motion mo; mo.add(I, 0.0); mo.add(I, 1.0);
        const std::vector<float> in = {1, 2, 3, 4, 0.5f, 0, 0, 0};
        const std::vector<float> tm = {0.5f};
        const float inf = std::numeric_limits<float>::infinity();
        struct R { const char* name; const char* field; dsk::Call c; Motion mo; double t0, t_ref; };
        std::vector<R> cases;
        const dsk::Call good{in.data(), 1, 16, tm.data(), PCR_TIME_F32_SECONDS, 0, nullptr, nullptr, true};
        auto add = [&](const char* name, const char* field) -> R& { cases.push_back(R{name, field, good, mo, 0.0, 0.0}); return cases.back(); };
        { R& r = add("K = 1", "K"); r.mo.poses.resize(16); r.mo.stamps.resize(1); }
        { R& r = add("K = 1025", "K"); r.mo.poses.assign(16 * 1025, 0.0); r.mo.stamps.resize(1025); for (int j = 0; j < 1025; ++j) { r.mo.stamps[j] = j; for (int d = 0; d < 4; ++d) r.mo.poses[16 * j + 5 * d] = 1; } }
        { R& r = add("stamps equal", "stamps"); r.mo.stamps[1] = 0.0; }
        { R& r = add("stamps decreasing", "stamps"); r.mo.stamps[1] = -1.0; }
        { R& r = add("stamp not finite", "stamps"); r.mo.stamps[1] = inf; }
        { R& r = add("pose not finite", "poses"); r.mo.poses[20] = NAN; }
        { R& r = add("pose without a unit quaternion", "poses"); for (int d = 0; d < 3; ++d) r.mo.poses[5 * d] = 1e308; }
        { R& r = add("t0 not finite", "t0"); r.t0 = NAN; }
        { R& r = add("t_ref not finite", "t_ref"); r.t_ref = inf; }
        { R& r = add("time_kind", "time_kind"); r.c.kind = 3; }
        { R& r = add("stride 12", "stride_bytes"); r.c.stride = 12; }
        { R& r = add("offset misaligned", "time_offset_bytes"); r.c.times = nullptr; r.c.stride = 32; r.c.off = 18; }
        { R& r = add("offset past the stride", "time_offset_bytes"); r.c.times = nullptr; r.c.stride = 32; r.c.off = 32; }
        { R& r = add("offset in the coordinates", "time_offset_bytes"); r.c.times = nullptr; r.c.stride = 32; r.c.off = 8; }
        { R& r = add("double past the stride", "time_offset_bytes"); r.c.times = nullptr; r.c.stride = 28; r.c.off = 24; r.c.kind = PCR_TIME_F64_SECONDS; }
        { R& r = add("pts NULL", "pts"); r.c.pts = nullptr; }
        for (R& r : cases) {
            out.assign(4, -77.0f);
            r.c.out = out.data();
            r.c.m = r.mo.get(r.t0, r.t_ref);
            const char* why = dsk::deskew_host(r.c, &info);
            const bool ok = why && strstr(why, r.field) && out[0] == -77.0f && out[3] == -77.0f;
            report((std::string("refused: ") + r.name).c_str(), ok, why ? why : "accepted");
        }
        out.assign(8, -77.0f);
        dsk::Call c = good;
        c.m = nullptr; c.out = out.data();
        const char* why = dsk::deskew_host(c, &info);
        report("refused: m NULL", why && strstr(why, "m is NULL"));
        c.m = mo.get(0.0, 0.0); c.out = nullptr;
        why = dsk::deskew_host(c, &info);
        report("refused: out NULL", why && strstr(why, "out"));
        std::vector<float> two = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
        const std::vector<float> keep = two;
        const std::vector<float> tm2 = {0.5f, 0.5f};
        c = dsk::Call{two.data(), 2, 16, tm2.data(), PCR_TIME_F32_SECONDS, 0, mo.get(0.0, 0.0), two.data() + 4, true};
        why = dsk::deskew_host(c, &info);
        report("refused: partial overlap", why && strstr(why, "out") && two == keep);
        c.n = 0; c.pts = nullptr; c.out = nullptr;
        why = dsk::deskew_host(c, &info);
        report("n = 0", !why && info.before == 0 && info.nonfinite == 0);
    }
    printf("%d failed\n", g_failed);
    return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "--self") return self_check();
    fprintf(stderr, "usage: deskew_check --self\n");
    return 2;
}
