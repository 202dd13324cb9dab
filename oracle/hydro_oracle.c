/*
 * CPU oracle, plain C, float64 - TEST INFRASTRUCTURE ONLY.
 *
 * A scalar, one-body-per-call restatement of the reference's Numba path, used
 * (a) as a second, independent checker beside oracle/hydro_oracle.py and
 * (b) as the "port" CPU baseline timed by bench.py on the GPU box's host cores
 *     (the reference's Python files never travel and Numba is not installed).
 * Nothing under silver2_isaacsim_amd/ links or loads this file.
 *
 * Follows, function by function:
 *   quat_to_rot            numba_hydrodynamics.py:9-51
 *   submersion_and_cob     numba_hydrodynamics.py:54-105   (27 world keypoints,
 *                          lattice of numba_hydrodynamics_wrapper.py:55-73)
 *   pressure_and_area      numba_hydrodynamics.py:108-143  (faces of wrapper :75-99)
 *   hybrid_drag            numba_hydrodynamics.py:146-182
 *   lift                   numba_hydrodynamics.py:185-217
 *   added_mass             numba_hydrodynamics.py:220-253  (diag of wrapper :101-112)
 *   solve_body             numba_hydrodynamics.py:256-314
 *   epilogue               hydrodynamics_behavior.py:196-202,212-226
 * N1 completion (speed <= 1e-6 -> cop = cob, area = 0): see hydro_oracle.py.
 *
 * Pinned by tests/test_oracle_golden.py against tests/golden/*.npz, which hold
 * outputs of the reference itself.  Build: oracle/Makefile (-O3 -ffast-math
 * mirrors @njit(fastmath=True)).
 * Finite inputs only: -ffast-math lets the compiler assume that no value is a NaN or an infinity, so what this file returns
 * for a non-finite constant is not defined by its source.  tests/test_oracle_golden.py holds it to the rows of
 * tests/golden/parameter_cases.npz on which the reference is finite; the rule for the others is hydro_oracle.py's.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef struct { double x, y, z; } v3;

static inline v3 v3_make(double x, double y, double z) { v3 r = {x, y, z}; return r; }
static inline v3 v3_add(v3 a, v3 b) { return v3_make(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline v3 v3_sub(v3 a, v3 b) { return v3_make(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 v3_scale(v3 a, double s) { return v3_make(a.x * s, a.y * s, a.z * s); }
static inline double v3_dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline double v3_norm(v3 a) { return sqrt(v3_dot(a, a)); }
static inline v3 v3_cross(v3 a, v3 b) {
    return v3_make(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

typedef struct { double m[3][3]; } m3;

static inline v3 m3_mul(const m3 *r, v3 a) {
    return v3_make(r->m[0][0] * a.x + r->m[0][1] * a.y + r->m[0][2] * a.z,
                   r->m[1][0] * a.x + r->m[1][1] * a.y + r->m[1][2] * a.z,
                   r->m[2][0] * a.x + r->m[2][1] * a.y + r->m[2][2] * a.z);
}
static inline v3 m3_tmul(const m3 *r, v3 a) {   /* R^T a */
    return v3_make(r->m[0][0] * a.x + r->m[1][0] * a.y + r->m[2][0] * a.z,
                   r->m[0][1] * a.x + r->m[1][1] * a.y + r->m[2][1] * a.z,
                   r->m[0][2] * a.x + r->m[1][2] * a.y + r->m[2][2] * a.z);
}

static m3 quat_to_rot(const double q[4]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double x2 = x + x, y2 = y + y, z2 = z + z;
    const double xx = x * x2, xy = x * y2, xz = x * z2;
    const double yy = y * y2, yz = y * z2, zz = z * z2;
    const double wx = w * x2, wy = w * y2, wz = w * z2;
    m3 r;
    r.m[0][0] = 1.0 - (yy + zz); r.m[0][1] = xy - wz;         r.m[0][2] = xz + wy;
    r.m[1][0] = xy + wz;         r.m[1][1] = 1.0 - (xx + zz); r.m[1][2] = yz - wx;
    r.m[2][0] = xz - wy;         r.m[2][1] = yz + wx;         r.m[2][2] = 1.0 - (xx + yy);
    return r;
}

typedef struct {
    v3 buoy, drag_f, lift_f, drag_t, am_f, am_t, cob, cop;
    double ratio;
} body_out;

/* one body; params = dimx dimy dimz cd_lin cd_ang damp_lin damp_ang lift am_lin am_ang mass */
static body_out solve_body(v3 p, const double q[4], v3 v, v3 w, v3 a, v3 alpha,
                           const double *prm, double rho, double g)
{
    body_out o;
    memset(&o, 0, sizeof o);
    const double dx = prm[0], dy = prm[1], dz = prm[2];
    const double hx = 0.5 * dx, hy = 0.5 * dy, hz = 0.5 * dz;
    const double volume = dx * dy * dz;
    const m3 rot = quat_to_rot(q);

    /* --- 27 world keypoints: extent + mean of the wet ones --- */
    double z_lo = 1e300, z_hi = -1e300;   /* finite sentinels: built with -ffast-math */
    v3 wet_sum = v3_make(0, 0, 0);
    int n_wet = 0;
    for (int k = 1; k >= -1; --k)
        for (int j = 1; j >= -1; --j)
            for (int i = -1; i <= 1; ++i) {
                v3 pt = v3_add(m3_mul(&rot, v3_make(i * hx, j * hy, k * hz)), p);
                if (pt.z < z_lo) z_lo = pt.z;
                if (pt.z > z_hi) z_hi = pt.z;
                if (pt.z < 0.0) { wet_sum = v3_add(wet_sum, pt); ++n_wet; }
            }
    double ratio;
    v3 cob = p;
    if (z_lo >= 0.0) ratio = 0.0;
    else if (z_hi <= 0.0) ratio = 1.0;
    else {
        const double height = z_hi - z_lo;
        if (height < 1e-6) ratio = (z_lo < 0.0) ? 1.0 : 0.0;
        else { ratio = -z_lo / height; if (ratio > 1.0) ratio = 1.0; }
        if (n_wet > 0) cob = v3_scale(wet_sum, 1.0 / n_wet);
    }
    if (ratio <= 1e-9) return o;                    /* dry: everything zero, cob/cop too */
    o.ratio = ratio;
    o.cob = cob;
    o.buoy = v3_make(0.0, 0.0, rho * (ratio * volume) * g);

    const double speed = v3_norm(v);
    const int moving = speed > 1e-6;
    const v3 vdir = moving ? v3_scale(v, 1.0 / speed) : v3_make(0, 0, 0);

    /* --- centre of pressure / projected area over the 6 faces --- */
    double area = 0.0;
    v3 cop = cob;
    if (moving) {
        const double half[3] = {hx, hy, hz};
        const double farea[3] = {dy * dz, dx * dz, dx * dy};
        v3 weighted = v3_make(0, 0, 0);
        for (int ax = 0; ax < 3; ++ax)
            for (int s = 1; s >= -1; s -= 2) {
                v3 nl = v3_make(0, 0, 0), cl = v3_make(0, 0, 0);
                ((double *)&nl)[ax] = (double)s;
                ((double *)&cl)[ax] = s * half[ax];
                const v3 nw = m3_mul(&rot, nl);
                const v3 cw = v3_add(m3_mul(&rot, cl), p);
                const double alignment = -v3_dot(nw, vdir);
                if (alignment > 0.0 && cw.z < 0.0) {
                    const double af = alignment * farea[ax];
                    area += af;
                    weighted = v3_add(weighted, v3_scale(cw, af));
                }
            }
        if (area > 1e-6) cop = v3_scale(weighted, 1.0 / area);
    }
    o.cop = cop;

    /* --- hybrid drag --- */
    {
        v3 quad = v3_make(0, 0, 0);
        if (moving) quad = v3_scale(vdir, -(0.5 * rho * (speed * speed) * prm[3] * area));
        const double s_lin = (speed < 0.2) ? speed / 0.2 : 1.0;
        o.drag_f = v3_scale(v3_sub(quad, v3_scale(v, prm[5] * s_lin)), ratio);
        const double wsp = v3_norm(w);
        v3 quad_t = v3_make(0, 0, 0);
        if (wsp > 1e-6) quad_t = v3_scale(v3_scale(w, 1.0 / wsp), -(0.5 * rho * (wsp * wsp) * prm[4] * volume));
        const double s_ang = (wsp < 0.2) ? wsp / 0.2 : 1.0;
        o.drag_t = v3_scale(v3_sub(quad_t, v3_scale(w, prm[6] * s_ang)), ratio);
    }

    /* --- lift --- */
    if (!(speed < 1e-6)) {
        const v3 up = v3_make(rot.m[0][2], rot.m[1][2], rot.m[2][2]);
        double d = -v3_dot(up, vdir);
        if (d > 1.0) d = 1.0; else if (d < -1.0) d = -1.0;
        const double cl = sin(2.0 * asin(d));
        const double mag = 0.5 * rho * (speed * speed) * cl * area * prm[7];
        const v3 axis = v3_cross(vdir, up);
        const double na = v3_norm(axis);
        if (!(na < 1e-6)) {
            const v3 dir = v3_cross(v3_scale(axis, 1.0 / na), vdir);
            o.lift_f = v3_scale(dir, mag * ratio);
        }
    }

    /* --- added mass: -diag(M) * body-frame acceleration, back to world --- */
    {
        const double lin = volume * prm[8] * rho;
        const double ax_ = volume * (dy * dy + dz * dz) * prm[9] * rho;
        const double ay_ = volume * (dx * dx + dz * dz) * prm[9] * rho;
        const double az_ = volume * (dx * dx + dy * dy) * prm[9] * rho;
        const v3 ab = m3_tmul(&rot, a), alb = m3_tmul(&rot, alpha);
        o.am_f = v3_scale(m3_mul(&rot, v3_make(-lin * ab.x, -lin * ab.y, -lin * ab.z)), ratio);
        o.am_t = v3_scale(m3_mul(&rot, v3_make(-ax_ * alb.x, -ay_ * alb.y, -az_ * alb.z)), ratio);
    }
    return o;
}

static inline void put3(double *dst, v3 a) { dst[0] = a.x; dst[1] = a.y; dst[2] = a.z; }

/* components for n bodies; state n x 13, accel n x 6, params n x 11 (row-major, f64);
 * comps n x 24 in the reference's output order, ratio n. */
int hydro_oracle_components(int64_t n, const double *state, const double *accel, const double *params,
                            double rho, double g, double *comps, double *ratio)
{
    for (int64_t i = 0; i < n; ++i) {
        const double *s = state + 13 * i, *ac = accel + 6 * i;
        const body_out o = solve_body(v3_make(s[0], s[1], s[2]), s + 3, v3_make(s[7], s[8], s[9]),
                                      v3_make(s[10], s[11], s[12]), v3_make(ac[0], ac[1], ac[2]),
                                      v3_make(ac[3], ac[4], ac[5]), params + 11 * i, rho, g);
        double *c = comps + 24 * i;
        put3(c + 0, o.buoy); put3(c + 3, o.drag_f); put3(c + 6, o.lift_f); put3(c + 9, o.drag_t);
        put3(c + 12, o.am_f); put3(c + 15, o.am_t); put3(c + 18, o.cob); put3(c + 21, o.cop);
        ratio[i] = o.ratio;
    }
    return 0;
}

/* fused path (A13 + A1-A11 + A14 + A15) on fp32 inputs, as the wrapper receives them
 * (numba_hydrodynamics_wrapper.py:40-45 casts to float64 per call).  threads<=1: scalar loop. */
int hydro_oracle_wrench(int64_t n, const float *state, const float *prev, const float *params,
                        double rho, double g, double dt, double *net_f, double *net_t, int threads)
{
    (void)threads;
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(threads > 1 ? threads : 1)
#endif
    for (int64_t i = 0; i < n; ++i) {
        double s[13], prm[11];
        for (int k = 0; k < 13; ++k) s[k] = (double)state[13 * i + k];
        for (int k = 0; k < 11; ++k) prm[k] = (double)params[11 * i + k];
        const v3 p = v3_make(s[0], s[1], s[2]);
        const v3 v = v3_make(s[7], s[8], s[9]), w = v3_make(s[10], s[11], s[12]);
        const v3 a = v3_scale(v3_sub(v, v3_make(prev[6 * i + 0], prev[6 * i + 1], prev[6 * i + 2])), 1.0 / dt);
        const v3 al = v3_scale(v3_sub(w, v3_make(prev[6 * i + 3], prev[6 * i + 4], prev[6 * i + 5])), 1.0 / dt);
        const body_out o = solve_body(p, s + 3, v, w, a, al, prm, rho, g);
        const v3 arm_b = v3_sub(o.cob, p), arm_p = v3_sub(o.cop, p);
        v3 f = v3_add(v3_add(o.buoy, o.drag_f), v3_add(o.lift_f, o.am_f));
        v3 t = v3_add(v3_add(v3_cross(arm_b, o.buoy), v3_cross(arm_p, o.drag_f)),
                      v3_add(v3_cross(arm_p, o.lift_f), v3_add(o.drag_t, o.am_t)));
        double scale = prm[10] * 500.0 / (v3_norm(f) + 1e-6);
        if (scale > 1.0) scale = 1.0;
        put3(net_f + 3 * i, v3_scale(f, scale));
        put3(net_t + 3 * i, v3_scale(t, scale));
    }
    return 0;
}

int hydro_oracle_max_threads(void)
{
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}
