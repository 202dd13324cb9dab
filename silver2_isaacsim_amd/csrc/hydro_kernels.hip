// gfx950 (MI355X / CDNA4) kernels and C ABI of libhydro.so - see include/hydro.h.
//
// Every kernel is elementwise per rigid body: about 460 VALU instructions, two thirds of them fp64 (hydro_body.h says
// why), against 122-144 B per body-step - no MFMA anywhere.  The wrench kernels are CO-LIMITED: a memory-only probe of
// the traffic takes 20.5 us and a compute-only probe of the arithmetic 16 us at 1 M bodies, each at the ~2.4 GHz the chip
// holds for it alone; doing both it holds ~2.0 GHz, where the arithmetic takes as long as the bytes (scripts/probes.py,
// DESIGN.md section 6; kernel 21.4 us).  What matters is
//   * layouts in which each wave-instruction reads one contiguous 256-B run of one field
//     (plain SoA) and - better - in which the ~28 runs a wavefront needs form three contiguous
//     records (tiled SoA, the native layout): DRAM pages are consumed whole;
//   * all of a body's 28 loads issued before the first use, so a wave has its whole working
//     set in flight at once (single-pass kernels, latency hidden by 4 waves per SIMD: 101-115 VGPRs);
//   * instruction count: every VALU instruction but fp32 arithmetic costs ~4 cycles per wave here, fp64 or not;
//   * streaming accesses for scenes larger than the caches (every byte is touched once per step): non-temporal loads,
//     and WRITE-THROUGH stores - an nt store parks its dirty line in L2, a write-through one hands it on (see stg);
//   * nothing re-read and nothing written but the wrench (24 B per body).
// The array-of-structs entry (the simulator's tensor layout) reads and writes one row per lane with 12- and 16-byte
// accesses (LDS staging of the transposition was measured and lost: DESIGN.md section 5); the kinetic-energy
// reduction - stand-alone, or fused into the wrench / step kernels for the bodies already in registers - is where lanes
// exchange data: LDS across the block's four waves, wave64 DPP butterflies, and integer tickets that let ONE launch
// finish the fixed-order sum (see "kinetic-energy reduction" below).  One code path per kernel: the forms that were
// measured and rejected live in scripts/ab/.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <dlfcn.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include <mutex>
#include <new>
#include <type_traits>

#include "../../include/hydro.h"
#include "hydro_body.h"
#include "hydro_watch.h"

// The tiled wrench kernel is built for AT MOST 4 waves per SIMD.  After the instruction diet of round 3 two of its
// instantiations need only 95 VGPRs and would run 5 waves per SIMD; interleaved A/B on three boxes:
// the same code at 4 waves is 0.1-0.3 us faster at 1 M bodies (22.31-22.56 vs 22.39-22.86 us) - the fifth wave buys no
// latency hiding that the kernel lacks and costs a little in the memory system.
#define HYDRO_TILED_OCC_ATTR __attribute__((amdgpu_waves_per_eu(1, 4)))

namespace {

constexpr int kBlock = 256;                // 4 waves of 64 lanes
// Occupancy: the fp64 body needs 98-132 VGPRs depending on the kernel around it and on the build flags, i.e. 3-4 waves
// per SIMD.  Forcing a number (__launch_bounds__' second argument) made the compiler spill 2-4 registers on the path
// every wave runs when the kernel needed 130: measured 28.2 vs 24.0 us at 1 M bodies - the
// kernels are left at what they need.

// --------------------------------------------------------------------------
// vector load / store helpers: VEC consecutive bodies of one SoA field per lane
// --------------------------------------------------------------------------
// `i` is a 32-bit ELEMENT index; the byte offset is formed in 32 bits on purpose so that the
// access compiles to the "SGPR base + 32-bit VGPR offset" addressing form (no 64-bit per-lane
// address arithmetic, no VGPR pairs for addresses).  hydro_create caps capacity at 2^30.
template <typename T>
__device__ __forceinline__ const T* at(const void* __restrict__ p, uint32_t byte_off)
{
    return reinterpret_cast<const T*>(static_cast<const char*>(p) + byte_off);
}
template <typename T>
__device__ __forceinline__ T* at(void* __restrict__ p, uint32_t byte_off)
{
    return reinterpret_cast<T*>(static_cast<char*>(p) + byte_off);
}

// base + per-lane offset + compile-time field offset.  The field offset is added AFTER the 32-bit lane offset
// has been zero-extended (pointer arithmetic), so it lands in the load instruction's immediate
// (global_load_dword v, voff, s[base] offset:f*256); written as `voff + f*256` in 32 bits the compiler must
// keep the wrap-around semantics and spends one v_add_u32 + one VGPR per field.
template <typename T>
__device__ __forceinline__ const T* at(const void* __restrict__ p, uint32_t lane_off, uint32_t field_off)
{
    return reinterpret_cast<const T*>(static_cast<const char*>(p) + lane_off + field_off);
}
template <typename T>
__device__ __forceinline__ T* at(void* __restrict__ p, uint32_t lane_off, uint32_t field_off)
{
    return reinterpret_cast<T*>(static_cast<char*>(p) + lane_off + field_off);
}

// NT = streaming access: every byte of a large scene is touched once per step, so nothing is worth keeping in
// L2 / Infinity Cache: non-temporal loads (measured +5..9 % on the SoA kernel) and write-through stores (below).
template <bool NT, typename V>
__device__ __forceinline__ V ldg(const V* p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
// Streaming STORES are write-through (`sc0 sc1`), not `nt`.  An nt store leaves its line dirty in the XCD's L2 to be
// written back later (MI355X_MICROARCH.md: "plain / sc0 / nt KEEP the line in L2, sc1 / sc0 sc1 DROP it"); a kernel
// that writes 24-48 B per body and never reads them again does better handing them straight to the memory side.
// Measured, sustained over 2 s per variant on two boxes (scripts/ab_sustained.py, C5): nt 22.83-23.09 / 23.5-25.1 us,
// sc1 21.44 / 22.8-24.0, sc0 sc1 21.36 / 22.15-22.5 us per launch (-6.5 %); 4 M bodies 80.9 -> 79.0 us; identical bits.
// One write-through store of 4 or 8 bytes (all the streaming kernels need: one field of one or two bodies per lane).  The
// compiler offers the cache policy only through atomics.
template <typename V>
__device__ __forceinline__ void store_write_through(V* p, V v)
{
    static_assert(sizeof(V) == 4 || sizeof(V) == 8, "one or two floats");
    if constexpr (sizeof(V) == 4) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The simulator-facing AoS kernel is the exception: its 12-byte force / torque rows and its prev-velocity fields measured
// 2-3 % FASTER as nt stores (27.75 vs 28.32 us at 1 M bodies, 102.0 vs 105.1 us at 4 M), so it stays on stg_nt.
template <bool NT, typename V>
__device__ __forceinline__ void stg_nt(V* p, V v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}
template <bool NT, typename V>
__device__ __forceinline__ void stg(V* p, V v)
{
    if constexpr (NT) store_write_through(p, v);
    else *p = v;
}

template <int VEC, bool NT>
__device__ __forceinline__ void load_f32(const float* __restrict__ p, uint32_t i, float (&out)[VEC])
{
    if constexpr (VEC == 1) {
        out[0] = ldg<NT>(at<float>(p, i * 4u));
    } else {
        static_assert(VEC == 2, "SoA kernels are built for 1 or 2 bodies per lane");
        using V2 = float __attribute__((ext_vector_type(2)));
        const V2 v = ldg<NT>(at<V2>(p, i * 4u));
        out[0] = v.x; out[1] = v.y;
    }
}

template <int VEC, bool NT>
__device__ __forceinline__ void store_f32(float* __restrict__ p, uint32_t i, const float (&in)[VEC])
{
    if constexpr (VEC == 1) {
        stg<NT>(at<float>(p, i * 4u), in[0]);
    } else {
        using V2 = float __attribute__((ext_vector_type(2)));
        V2 v; v.x = in[0]; v.y = in[1];
        stg<NT>(at<V2>(p, i * 4u), v);
    }
}

__device__ __forceinline__ float half_bits_to_float(unsigned short b) { return __half2float(__ushort_as_half(b)); }

template <int VEC, bool NT>
__device__ __forceinline__ void load_f16(const __half* __restrict__ p, uint32_t i, float (&out)[VEC])
{
    if constexpr (VEC == 1) {
        out[0] = half_bits_to_float(ldg<NT>(at<unsigned short>(p, i * 2u)));
    } else {
        const unsigned int raw = ldg<NT>(at<unsigned int>(p, i * 2u));
        out[0] = half_bits_to_float((unsigned short)(raw & 0xffffu));
        out[1] = half_bits_to_float((unsigned short)(raw >> 16));
    }
}

template <int VEC, bool HALF, bool NT>
__device__ __forceinline__ void load_coef(const void* __restrict__ p, uint32_t i, float (&out)[VEC])
{
    if constexpr (HALF) load_f16<VEC, NT>(static_cast<const __half*>(p), i, out);
    else load_f32<VEC, NT>(static_cast<const float*>(p), i, out);
}

template <bool HALF>
__device__ __forceinline__ float load_coef1(const void* __restrict__ p, uint32_t i)
{
    if constexpr (HALF) return __half2float(*at<__half>(p, i * 2u));
    else return *at<float>(p, i * 4u);
}


// --------------------------------------------------------------------------
// kinetic-energy reduction ("wave64 shuffle/DPP -> LDS -> one fp64 partial per block -> deterministic second
// stage"), all of it inside ONE launch.
//
// The first stage is the same code whether it runs stand-alone (ke_kernel) or inside a wrench / step kernel that has the
// bodies in registers anyway (their KE template argument), so both give the same bits:
//   1. one block = one GROUP of 256 consecutive bodies, wave w holds tile w in its lanes (a lane without a body holds
//      +0.0).  The four waves' lane values meet in LDS; lane l of wave 0 adds ITS four bodies in order,
//      x_l = ((b0 + b1) + b2) + b3, and waves 1-3 are done;
//   2. wave 0 adds its 64 lane sums (wave_sum below: DPP butterflies inside the rows of 16, then the four rows in order)
//      -> partial P_g, published at partials[g];
//   3. groups are dealt to 64 CLASSES round-robin, class(g) = g % 64.  The class sum S_c adds the partials of class c in a
//      fixed order (lane t of ONE wavefront takes the class's members t, t + 64, t + 128, ... in that order, absent ones as +0.0; then wave_sum), the total adds
//      S_0 .. S_63 through one more wave_sum.
// Who does step 3 is decided by TICKETS (integer atomics; no floating-point atomics anywhere): wave 0 of every block
// draws one from its class's counter, the one that draws a class's last ticket adds that class and draws from the top
// counter, the one that draws the last of those adds the classes.  Two levels because a device-scope atomic on ONE
// address costs ~12 ns per ticket, SERIALISED (scripts/ubench_atomics.hip: 48 us for the 4 096 blocks of 1 M bodies on one
// counter; the same tickets spread over 32 counters cost nothing measurable), and because the final sum is split over up
// to 64 wavefronts.  The result does not depend on which block draws which ticket.
// Memory ordering is spelled out for gfx950 rather than asked of the compiler as release / acquire at device scope:
// a release there is a write-back of the whole L2 (buffer_wbl2; measured 7 ns per fence, serialised over the device - 30 us
// for the blocks of 1 M bodies) and exists to publish ORDINARY stores.  Here everything that crosses blocks is a
// device-scope atomic access - write-through stores (sc1), sc1 loads, the tickets - with s_waitcnt vmcnt(0) between a
// wave's stores and its ticket ("complete" at device scope), and the few wavefronts that read what others wrote
// invalidate their non-coherent caches first (one buffer_inv per finisher: at most 65 per launch).
// What the tail costs: ~0.75 us per ticket whose result is waited for, ~0.2 us per published value, i.e. ~2.5 us after the
// last block's bodies have arrived; a second launch for the final sum cost 4 us.
// The counters are reset by the wavefronts that finish, so a launch leaves them at 0: launches on one engine must not
// overlap (a handle is not thread-safe anyway; the host side orders a launch on a NEW stream behind the previous one, see
// ke_prepare).  A launch that does not run to its end (a device reset, an aborted graph) leaves counters behind on which no
// later launch draws the "last" ticket.  So that this cannot pass for a result, block 0 POISONS `out` with NaNs before it
// draws its ticket - ordered before the final store through the ticket chain, both write-through - and only a launch
// that finishes overwrites them; the host re-arms the counters (hydro_ke_rearm, and by itself after any HIP error seen
// on the handle).  The other shape of that fault - a class counter left at 0 < k < members, so that a later launch's
// finisher adds its class k blocks too early - meets the second poison: every class finisher overwrites the partials it
// has consumed with NaNs, so the slots the early finisher finds unwritten hold NaNs from the last launch that finished,
// and the total is NaN.  What is NOT covered: slots the unfinished launch itself had published before it died (finite,
// stale if the scene changed since) - a launch that dies without the library seeing a HIP error and without taking the
// process with it; hydro_ke_rearm is the answer to that, the poison is not.
// Scratch (doubles): [stride] translational partials | [stride] rotational | [64] + [64] class sums | counters (uint32, one
// per 256 B): top, class 0 .. 63.
// --------------------------------------------------------------------------
constexpr uint32_t kKeClasses = 64;
constexpr size_t kKeScratchTailBytes = 2 * kKeClasses * sizeof(double) + (1 + kKeClasses) * 256;

// Sum over the 64 lanes of a wavefront, the same bits in whatever order the hardware runs: inside each row of 16 lanes
// four butterfly steps on DPP moves (lane ^ 1, lane ^ 2, mirror of 8, mirror of 16: a + b == b + a, so every lane of a
// row ends up with the same row sum), then the four row sums in order, ((r0 + r1) + r2) + r3, read with v_readlane.
// ~25 instructions and no LDS round trips (the ds_bpermute tree it replaces: twelve dependent ones for a pair).
template <int CTRL>
__device__ __forceinline__ double dpp_move(double x)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double read_lane(double x, int lane)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum(double x)          // every lane of the wavefront must be active
{
    x += dpp_move<0xB1>(x);        // quad_perm [1,0,3,2]
    x += dpp_move<0x4E>(x);        // quad_perm [2,3,0,1]
    x += dpp_move<0x141>(x);       // row_half_mirror
    x += dpp_move<0x140>(x);       // row_mirror
    return ((read_lane(x, 0) + read_lane(x, 16)) + read_lane(x, 32)) + read_lane(x, 48);
}
__device__ __forceinline__ void ke_publish(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ke_fetch(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// lane 0 draws a ticket; every lane gets its number
__device__ __forceinline__ uint32_t ke_ticket(uint32_t* counter)
{
    uint32_t t = 0;
    if (threadIdx.x == 0) t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __builtin_amdgcn_readfirstlane(t);
}
__device__ __forceinline__ void ke_reset(uint32_t* counter)
{
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Every thread of a 256-thread block calls this with the kinetic energy of its body (zeros for a lane without one).
// `groups` == gridDim.x.
__device__ __forceinline__ void ke_block_reduce(double lin, double rot, double* __restrict__ scratch, uint32_t stride, double* __restrict__ out)
{
    __shared__ double stage[2][kBlock];
    stage[0][threadIdx.x] = lin;
    stage[1][threadIdx.x] = rot;
    if (blockIdx.x == 0 && threadIdx.x == 0) {                  // no result yet: NaNs until the last ticket of all replaces them
        ke_publish(out, __builtin_nan(""));
        ke_publish(out + 1, __builtin_nan(""));
    }
    __syncthreads();
    if (threadIdx.x >= 64u) return;                              // waves 1-3 are done
    // ---- wave 0, all 64 lanes, no barrier from here on ----
    const uint32_t l = threadIdx.x, group = blockIdx.x, groups = gridDim.x;
    double a = ((stage[0][l] + stage[0][64 + l]) + stage[0][128 + l]) + stage[0][192 + l];       // step 1
    double b = ((stage[1][l] + stage[1][64 + l]) + stage[1][128 + l]) + stage[1][192 + l];
    a = wave_sum(a);                                                                             // step 2
    b = wave_sum(b);
    if (l == 0) { ke_publish(scratch + group, a); ke_publish(scratch + stride + group, b); }
    double* class_sums = scratch + 2 * (size_t)stride;
    uint32_t* counters = reinterpret_cast<uint32_t*>(class_sums + 2 * kKeClasses);
    const uint32_t cls = group % kKeClasses;
    const uint32_t members = (groups - cls + kKeClasses - 1u) / kKeClasses;                      // groups g < groups with g % 64 == cls
    __builtin_amdgcn_s_waitcnt(0);                               // the partial is complete at device scope before the ticket goes out
    if (ke_ticket(counters + 64u * (1u + cls)) != members - 1u) return;
    // ---- the last ticket of the class: S_cls (step 3, first half) ----
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    a = 0.0; b = 0.0;
    for (uint32_t e0 = 0; e0 < members; e0 += 256u) {           // four members per lane in flight (4 M bodies: one round)
        double pa[4], pb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t e = e0 + 64u * k + l;
            pa[k] = e < members ? ke_fetch(scratch + cls + kKeClasses * e) : 0.0;
            pb[k] = e < members ? ke_fetch(scratch + stride + cls + kKeClasses * e) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { a += pa[k]; b += pb[k]; }
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (l == 0) { ke_publish(class_sums + cls, a); ke_publish(class_sums + kKeClasses + cls, b); }
    ke_reset(counters + 64u * (1u + cls));
    const uint32_t classes = groups < kKeClasses ? groups : kKeClasses;
    __builtin_amdgcn_s_waitcnt(0);
    if (ke_ticket(counters) == classes - 1u) {
        // ---- and the last ticket of all: the total ----
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        a = l < classes ? ke_fetch(class_sums + l) : 0.0;
        b = l < classes ? ke_fetch(class_sums + kKeClasses + l) : 0.0;
        a = wave_sum(a);
        b = wave_sum(b);
        if (l == 0) { ke_publish(out, a); ke_publish(out + 1, b); }
        ke_reset(counters);
    }
    // The partials this wavefront has consumed: leave NaNs behind (same-address atomics stay in program order).  Should a
    // LATER launch ever add a class before all of its members have published - ticket counters an unfinished launch left at
    // 0 < k < members and the library did not see (ke_suspect) - what it finds in the missing slots is a NaN, not this
    // launch's pair.  The LAST thing a class finisher does: nothing in this launch waits for these stores (ahead of the top
    // ticket, that ticket's s_waitcnt held every class back by their round trip: 14.2 instead of 13.3 us at 1 M bodies; ahead
    // of the total, the acquire fence waits for them); the end of the kernel completes them before the next launch publishes
    // into the same slots.
    for (uint32_t e = l; e < members; e += 64u) {
        ke_publish(scratch + cls + kKeClasses * e, __builtin_nan(""));
        ke_publish(scratch + stride + cls + kKeClasses * e, __builtin_nan(""));
    }
}

// --------------------------------------------------------------------------
// kernel arguments (passed by value in the kernarg segment: pointers land in SGPRs)
// --------------------------------------------------------------------------
struct SoaArgs {
    const float* st[HYDRO_STATE_FIELDS];
    const float* pv[HYDRO_PREV_FIELDS];      // previous velocity (read)
    float* pv_out[HYDRO_PREV_FIELDS];        // where to store this step's velocity (WRITE_PREV)
    const float* dims[3];
    const void* coef[7];                     // float or __half
    const float* mass;
    float* out[HYDRO_WRENCH_FIELDS];
    double rho, g;                           // scene scalars stay fp64 up to the kernel (hydro_body.h)
    double inv_dt;                           // 1 / dt in fp64 (dt is a double through the C ABI)
    int warp;                                // HYDRO_SEM_WARP (uniform)
    int64_t n;
};

// One body from already-loaded scalars.
__device__ __forceinline__ hydro::BodyIn make_body(const float (&s)[HYDRO_STATE_FIELDS], const float (&d)[3], const float (&c)[7])
{
    hydro::BodyIn b;
    b.px = s[0]; b.py = s[1]; b.pz = s[2];
    b.qx = s[3]; b.qy = s[4]; b.qz = s[5]; b.qw = s[6];
    b.vx = s[7]; b.vy = s[8]; b.vz = s[9];
    b.wx = s[10]; b.wy = s[11]; b.wz = s[12];
    b.dimx = d[0]; b.dimy = d[1]; b.dimz = d[2];
    b.cd_lin = c[0]; b.cd_ang = c[1]; b.damp_lin = c[2]; b.damp_ang = c[3];
    b.lift = c[4]; b.am_lin = c[5]; b.am_ang = c[6];
    return b;
}

// A13 (finite-difference acceleration, hydrodynamics_behavior.py:200-202) + model + lever arms + sum + clamp
__device__ __forceinline__ hydro::Wrench body_wrench(const float (&s)[HYDRO_STATE_FIELDS], const float (&pv)[HYDRO_PREV_FIELDS],
                                                     const float (&d)[3], const float (&c)[7], float mass,
                                                     double rho, double g, double inv_dt, bool warp)
{
    return hydro::solve_wrench(make_body(s, d, c), pv, mass, rho, g, inv_dt, warp);
}
__device__ __forceinline__ void wrench_fields(const hydro::Wrench& w, float (&f6)[HYDRO_WRENCH_FIELDS])
{
    f6[0] = w.fx; f6[1] = w.fy; f6[2] = w.fz; f6[3] = w.tx; f6[4] = w.ty; f6[5] = w.tz;
}

// --------------------------------------------------------------------------
// fused wrench, struct-of-arrays.  Each lane owns VEC consecutive bodies.
// Algorithmic traffic per body: 52 B state + 24 B previous velocity + 44 B (30 B
// with fp16 coefficients) parameters in, 24 B wrench out (+24 B if WRITE_PREV).
// --------------------------------------------------------------------------
// WARP (every wrench kernel): the semantics of the reference's Warp twin (HYDRO_SEM_WARP) as a COMPILE-TIME switch.  As
// a run-time flag it cost the path everybody takes 12 v_cndmask_b32 (the compiler turns "R or R^T" into selects of the
// six off-diagonal matrix entries rather than branching around 18 multiply-adds).
template <int BLOCK, int VEC, bool HALF, bool WRITE_PREV, bool NT, bool WARP>
__global__ void __launch_bounds__(BLOCK) wrench_soa_kernel(const SoaArgs a)
{
    // Precondition (host side, launch_soa): a.n is a multiple of VEC; the <= VEC-1 leftover
    // bodies go to a second launch of the VEC=1 instance.  32-bit element offsets: the field
    // base pointers stay in SGPRs and every access is "saddr + 32-bit voffset".
    const uint32_t n = (uint32_t)a.n;
    const uint32_t base = (blockIdx.x * BLOCK + threadIdx.x) * VEC;
    if (base >= n) return;

    float st[HYDRO_STATE_FIELDS][VEC], pv[HYDRO_PREV_FIELDS][VEC], dm[3][VEC], cf[7][VEC], ms[VEC];
#pragma unroll
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) load_f32<VEC, NT>(a.st[f], base, st[f]);
#pragma unroll
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) load_f32<VEC, NT>(a.pv[f], base, pv[f]);
#pragma unroll
    for (int f = 0; f < 3; ++f) load_f32<VEC, NT>(a.dims[f], base, dm[f]);
#pragma unroll
    for (int f = 0; f < 7; ++f) load_coef<VEC, HALF, NT>(a.coef[f], base, cf[f]);
    load_f32<VEC, NT>(a.mass, base, ms);

    float out[HYDRO_WRENCH_FIELDS][VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        float s[HYDRO_STATE_FIELDS], p[HYDRO_PREV_FIELDS], d[3], c[7];
#pragma unroll
        for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) s[f] = st[f][j];
#pragma unroll
        for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) p[f] = pv[f][j];
#pragma unroll
        for (int f = 0; f < 3; ++f) d[f] = dm[f][j];
#pragma unroll
        for (int f = 0; f < 7; ++f) c[f] = cf[f][j];
        float f6[HYDRO_WRENCH_FIELDS];
        wrench_fields(body_wrench(s, p, d, c, ms[j], a.rho, a.g, a.inv_dt, WARP), f6);
#pragma unroll
        for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) out[f][j] = f6[f];
    }

#pragma unroll
    for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) store_f32<VEC, NT>(a.out[f], base, out[f]);
    if constexpr (WRITE_PREV) {
#pragma unroll
        for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) store_f32<VEC, NT>(a.pv_out[f], base, st[7 + f]);
    }
}

// --------------------------------------------------------------------------
// fused wrench, TILED struct-of-arrays (the engine's native layout).
//
// A field group with F fields over N bodies is stored as [ceil(N/64)][F][64] floats: inside a
// tile of 64 bodies (= one wavefront) every field is a contiguous 256-B run, and the tile's
// fields follow each other.  Body i, field f lives at  base[(i / 64) * tile_stride + f * 64 + i % 64].
// Coalescing is that of plain SoA (each wave-instruction still reads one 256-B run), but the
// ~28 runs a wave needs are now 3 contiguous records (3.3 KiB state, 1.5 KiB previous velocity,
// 2.75 KiB parameters) instead of 28 pieces scattered over 28 arrays: DRAM pages are used whole.
// Measured with memory-only probes at 4M bodies (round 1; the probes of this shape live in scripts/probes.py now):
// 6.1 TB/s against 5.4 TB/s for plain SoA, i.e. the float4-copy ceiling of the box.  All field offsets f*256 B fit the 12-bit
// immediate of global_load, so a wave needs ONE 32-bit offset register per record.
// --------------------------------------------------------------------------
// The engine's parameter record per tile is [dimx dimy dimz cd_lin cd_ang damp_lin damp_ang lift am_lin am_ang mass][64] f32, or
// with fp16 coefficients [dimx dimy dimz mass][64] f32 (1024 B) then the seven coefficients [64] f16 (896 B) = 1920 B = 480 floats.
constexpr uint32_t kPrmTileF32 = 11 * 64;
constexpr uint32_t kPrmTileF16 = 480;

// Dimensions, coefficients and mass of body (tile, lane) from the engine's parameter records (see load_tile_records).
template <bool HALF, bool NT>
__device__ __forceinline__ void load_param_record(const float* __restrict__ prm_all, uint32_t tile, uint32_t lane4,
                                                  float (&d)[3], float (&c)[7], float& mass)
{
    if constexpr (HALF) {
        const float* prm = prm_all + (size_t)tile * kPrmTileF16;
#pragma unroll
        for (int f = 0; f < 3; ++f) d[f] = ldg<NT>(at<float>(prm, lane4, f * 256u));
        mass = ldg<NT>(at<float>(prm, lane4, 3 * 256u));
        const uint32_t lane2 = lane4 >> 1;
#pragma unroll
        for (int f = 0; f < 7; ++f) c[f] = half_bits_to_float(ldg<NT>(at<unsigned short>(prm, lane2, 1024u + f * 128u)));
    } else {
        const float* prm = prm_all + (size_t)tile * kPrmTileF32;
#pragma unroll
        for (int f = 0; f < 3; ++f) d[f] = ldg<NT>(at<float>(prm, lane4, f * 256u));
#pragma unroll
        for (int f = 0; f < 7; ++f) c[f] = ldg<NT>(at<float>(prm, lane4, (3 + f) * 256u));
        mass = ldg<NT>(at<float>(prm, lane4, 10 * 256u));
    }
}
// state, previous velocity and parameter records of body (tile, lane): the ~28 loads of a wave are three
// contiguous records, every field offset in the load instruction's immediate.
// One wavefront = one tile, so the tile index is WAVE-UNIFORM: the callers hand it over as a scalar (wave_tile below) and
// the three record bases are scalar 64-bit adds; what is left per lane is ONE offset register for every 4-byte field of
// every record (lane * 4) and one for the fp16 coefficients (lane * 2) - 5 vector instructions of addressing per body where
// per-lane tile arithmetic (24-bit multiplies, add-shifts) took 15.  `st`, `pv` are the tile's records, not the buffers.
template <bool HALF, bool NT>
__device__ __forceinline__ void load_tile_records(const float* __restrict__ st, const float* __restrict__ pvr, const float* __restrict__ prm_all,
                                                  uint32_t tile, uint32_t lane4,
                                                  float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS],
                                                  float (&d)[3], float (&c)[7], float& mass)
{
#pragma unroll
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) s[f] = ldg<NT>(at<float>(st, lane4, f * 256u));
#pragma unroll
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) pv[f] = ldg<NT>(at<float>(pvr, lane4, f * 256u));
    load_param_record<HALF, NT>(prm_all, tile, lane4, d, c, mass);
}
// One field group of body (tile, lane) into its tiled record: v[0 .. F-1] to F consecutive 256-B runs.
template <int F, bool NT>
__device__ __forceinline__ void store_record(float* rec, uint32_t lane4, const float* v)
{
#pragma unroll
    for (int f = 0; f < F; ++f) stg<NT>(at<float>(rec, lane4, f * 256u), v[f]);
}
// The tile a wavefront works on, as a scalar: body i = block * BLOCK + thread with BLOCK a multiple of 64, so i >> 6 is
// the same in all 64 lanes - told to the compiler with v_readfirstlane on the wave-in-block index.
template <int BLOCK>
__device__ __forceinline__ uint32_t wave_tile(uint32_t block)
{
    static_assert(BLOCK % 64 == 0, "one wavefront = one tile");
    return block * (BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

// The wrench step of body (tile, lane), shared with the batch kernel, in two halves: records in, wrench computed; then the wrench
// and (WRITE_PREV) this step's velocity out.  Two, because the energy sample of a KE instantiation sits BETWEEN them in
// program order (behind the stores it costs the sampling kernels registers).
template <bool HALF, bool NT, bool WARP>
__device__ __forceinline__ void tile_wrench(const float* st, const float* pv_in, const float* prm, uint32_t st_stride, uint32_t pv_stride,
                                            uint32_t tile, uint32_t lane4, double rho, double g, double inv_dt,
                                            float (&s)[HYDRO_STATE_FIELDS], float (&d)[3], float& mass, float (&f6)[HYDRO_WRENCH_FIELDS])
{
    // tile < 2^24 and strides < 2^24, byte offsets < 2^32 (checked on the host)
    float pv[HYDRO_PREV_FIELDS], c[7];
    load_tile_records<HALF, NT>(st + (size_t)tile * st_stride, pv_in + (size_t)tile * pv_stride, prm, tile, lane4, s, pv, d, c, mass);
    wrench_fields(body_wrench(s, pv, d, c, mass, rho, g, inv_dt, WARP), f6);
}
template <bool WRITE_PREV, bool NT>
__device__ __forceinline__ void store_tile_wrench(float* out, float* pv_out, uint32_t out_stride, uint32_t pvo_stride, uint32_t tile, uint32_t lane4,
                                                  const float (&f6)[HYDRO_WRENCH_FIELDS], const float (&s)[HYDRO_STATE_FIELDS])
{
    store_record<HYDRO_WRENCH_FIELDS, NT>(out + (size_t)tile * out_stride, lane4, f6);
    if constexpr (WRITE_PREV) store_record<HYDRO_PREV_FIELDS, NT>(pv_out + (size_t)tile * pvo_stride, lane4, s + 7);
}

// The arguments are passed as individual scalars, the ones every wave needs before it can issue its first load in
// the first 16 dwords: with -mllvm -amdgpu-kernarg-preload-count=16 (build.py) those arrive in SGPRs with the wave
// (gfx950 kernarg preload) instead of behind three dependent scalar-memory round trips (~0.3 us per wave start,
// exposed in the ramp of every launch and in all of a 2.6 us launch).  A struct passed by value cannot be preloaded.
// KE = true (BLOCK 256 only): the kernel also samples the kinetic energy of the bodies it holds - the state it READS,
// i.e. the state after the previous step - and leaves one fp64 pair per block in `ke_partials` ([2][ke_stride]) for
// the fixed-order second stage: no second pass over the state ("reduced in-kernel").
// (The `int warp` argument of this and the other preloaded kernels is not read - WARP is the template argument - and stays:
// the argument lists are the kernarg-preload contract and part of the kernels' mangled names.)
template <int BLOCK, bool HALF, bool WRITE_PREV, bool NT, bool KE, bool WARP>
__global__ void __launch_bounds__(BLOCK) HYDRO_TILED_OCC_ATTR wrench_tiled_kernel(const float* k_st, const float* k_pv, const float* k_prm, float* k_out, float* k_pv_out,
                                                             uint32_t st_stride, uint32_t pv_stride, uint32_t out_stride, uint32_t pvo_stride,
                                                             uint32_t n, int warp, double rho, double g, double inv_dt,
                                                             double* ke_partials, uint32_t ke_stride, int ke_rotational, double* ke_out)
{
    const uint32_t tile = wave_tile<BLOCK>(blockIdx.x), lane = threadIdx.x & 63u;
    const uint32_t first = tile * 64u;                              // (scalar) bodies of this tile that exist: all 64 but in the last one
    // (scalar; written as n - min(n, first) through readfirstlane: as a saturating subtract the compiler moves it to the vector unit)
    const uint32_t left = n - __builtin_amdgcn_readfirstlane(n < first ? n : first);
    if constexpr (!KE) {
        if (lane >= left) return;
    }
    double ke_lin = 0.0, ke_rot = 0.0;
    if (!KE || lane < left) {                   // (KE: no early return - every thread reaches the block reduction)
        const uint32_t lane4 = lane * 4u;
        float s[HYDRO_STATE_FIELDS], d[3], mass, f6[HYDRO_WRENCH_FIELDS];
        tile_wrench<HALF, NT, WARP>(k_st, k_pv, k_prm, st_stride, pv_stride, tile, lane4, rho, g, inv_dt, s, d, mass, f6);
        if constexpr (KE)
            hydro::kinetic_energy(s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11], s[12], d[0], d[1], d[2], mass,
                                  ke_rotational != 0, ke_lin, ke_rot);
        store_tile_wrench<WRITE_PREV, NT>(k_out, k_pv_out, out_stride, pvo_stride, tile, lane4, f6, s);
    }
    if constexpr (KE) {
        static_assert(BLOCK == kBlock, "the kinetic-energy partials are one per 256 bodies");
        ke_block_reduce(ke_lin, ke_rot, ke_partials, ke_stride, ke_out);
    }
}

// --------------------------------------------------------------------------
// The same step for SEVERAL independent scenes in ONE launch (hydro_step_wrench_tiled_batch).  A launch pays a ramp (waves
// start, first bytes arrive) and a drain (the last waves finish alone) of ~1.5 us whatever its size: 7 % of a 1 M-body
// launch, under 2 % of a 4 M-body one (0.81 vs 0.89 of the HBM peak).  A caller that steps k replicas of a scene - the
// 1 024-environment style of config 3 - gets the big launch's efficiency without owning streams: the k scene descriptors
// travel in the kernarg segment, a block finds its scene from the prefix of block counts (scalar compares on two wide
// scalar loads) and loads that scene's descriptor with one more scalar load; from there on it is wrench_tiled_kernel's
// body on that scene's records - same arithmetic, same bits as k single launches.
// --------------------------------------------------------------------------
struct BatchScene {
    const float* st; const float* pv; const float* prm; float* out; float* pv_out;
    uint32_t st_stride, pv_stride, out_stride, pvo_stride;
    uint32_t n, pad;
    double rho, g;
};
// K = capacity of the kernarg table.  K = 4 (launches of up to four scenes): all four descriptors arrive with the FIRST
// round of scalar loads and the block's own is picked with scalar selects - one scalar-memory round trip before the first
// vector load instead of two (table, then descriptor); K = HYDRO_BATCH_MAX: the descriptor is loaded by index.
template <int K>
struct BatchArgs {
    uint32_t first_block[K];                    // first block of scene s in the grid (0xffffffff beyond the last scene)
    BatchScene sc[K];
    double inv_dt;
};
template <typename T> __device__ __forceinline__ T pick(bool c, T x, T y) { return c ? x : y; }

template <int K, bool HALF, bool WRITE_PREV, bool NT, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_TILED_OCC_ATTR wrench_tiled_batch_kernel(const BatchArgs<K> args)
{
    // first_block is increasing (0xffffffff beyond the last scene): the last j with first_block[j] <= block is the scene.
    // Everything here is uniform over the block - compares and selects on the scalar unit.
    const uint32_t bid = __builtin_amdgcn_readfirstlane(blockIdx.x);
    uint32_t scene = 0, first = args.first_block[0];
#pragma unroll
    for (int j = 1; j < K; ++j) {
        const bool here = bid >= args.first_block[j];
        scene = here ? (uint32_t)j : scene;
        first = here ? args.first_block[j] : first;
    }
    BatchScene b;
    if constexpr (K <= 4) {
        // what a wave needs before its first vector load, of ALL K scenes, asked for here: the scalar loads then go out
        // together with the table's (the compiler would otherwise sink them below the early exit: a second round trip)
#pragma unroll
        for (int j = 0; j < K; ++j)
            asm volatile("" : : "s"(args.sc[j].st), "s"(args.sc[j].pv), "s"(args.sc[j].prm), "s"(args.sc[j].st_stride), "s"(args.sc[j].pv_stride), "s"(args.sc[j].n));
        b = args.sc[0];
#pragma unroll
        for (int j = 1; j < K; ++j) {
            const bool m = scene == (uint32_t)j;
            const BatchScene& o = args.sc[j];
            b.st = pick(m, o.st, b.st); b.pv = pick(m, o.pv, b.pv); b.prm = pick(m, o.prm, b.prm); b.out = pick(m, o.out, b.out);
            b.pv_out = pick(m, o.pv_out, b.pv_out); b.st_stride = pick(m, o.st_stride, b.st_stride); b.pv_stride = pick(m, o.pv_stride, b.pv_stride);
            b.out_stride = pick(m, o.out_stride, b.out_stride); b.pvo_stride = pick(m, o.pvo_stride, b.pvo_stride);
            b.n = pick(m, o.n, b.n); b.rho = pick(m, o.rho, b.rho); b.g = pick(m, o.g, b.g);
        }
    } else {
        b = args.sc[scene];
    }
    const double inv_dt = args.inv_dt;          // (asked for here, ahead of the early exit, with the scene's scalars)
    const uint32_t tile = wave_tile<kBlock>(bid - first), lane = threadIdx.x & 63u, lane4 = lane * 4u;     // (wave-uniform, see load_tile_records)
    if (tile * 64u + lane >= b.n) return;
    float s[HYDRO_STATE_FIELDS], d[3], mass, f6[HYDRO_WRENCH_FIELDS];
    tile_wrench<HALF, NT, WARP>(b.st, b.pv, b.prm, b.st_stride, b.pv_stride, tile, lane4, b.rho, b.g, inv_dt, s, d, mass, f6);
    store_tile_wrench<WRITE_PREV, NT>(b.out, b.pv_out, b.out_stride, b.pvo_stride, tile, lane4, f6, s);
}

// Parameters: the caller's 11 field arrays -> the engine's tiled records (once per hydro_set_params_*), and back into
// plain-SoA copies for the entry points that take plain field pointers (made on their first use only).
struct ParamPtrs { const float* f[HYDRO_PARAM_FIELDS]; };
__global__ void __launch_bounds__(kBlock) params_to_tiled_kernel(const ParamPtrs src, float* __restrict__ tiled, int half, uint32_t n_pad, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_pad) return;
    const uint32_t tile = i >> 6, lane = i & 63u;
    const bool live = i < n;
    // padding lanes of the last tile get a benign unit box so that nothing in it is NaN
    float v[11];
#pragma unroll
    for (int f = 0; f < 11; ++f) v[f] = live ? src.f[f][i] : (f < 3 || f == 10 ? 1.0f : 0.0f);
    if (half) {
        float* rec = tiled + (size_t)tile * kPrmTileF16;
        rec[0 * 64 + lane] = v[0]; rec[1 * 64 + lane] = v[1]; rec[2 * 64 + lane] = v[2]; rec[3 * 64 + lane] = v[10];
        __half* hrec = reinterpret_cast<__half*>(rec + 256);
#pragma unroll
        for (int f = 0; f < 7; ++f) hrec[f * 64 + lane] = __float2half_rn(v[3 + f]);
    } else {
        float* rec = tiled + (size_t)tile * kPrmTileF32;
#pragma unroll
        for (int f = 0; f < 11; ++f) rec[f * 64 + lane] = v[f];
    }
}

// The fp16 record's one refusal (hydro_set_params_f16): a FINITE coefficient that __float2half_rn would store as +-Inf, that is
// |x| >= 65520 (the tie between 65504 and 2^16 rounds to even: to 2^16).  A NaN or an Inf given as such is neither.  *first_bad
// starts as all ones and ends as the smallest (body << 3 | coefficient) that overflows: one flag word for the host to read.
__global__ void __launch_bounds__(kBlock) params_f16_range_kernel(const ParamPtrs src, unsigned long long* __restrict__ first_bad, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int f = 0; f < 7; ++f) {
        const float a = fabsf(src.f[3 + f][i]);
        if (a >= 65520.0f && a < __builtin_inff()) {
            atomicMin(first_bad, ((unsigned long long)i << 3) | (unsigned long long)f);
            return;
        }
    }
}

__global__ void __launch_bounds__(kBlock) params_from_tiled_kernel(const float* __restrict__ tiled, int half, float* __restrict__ soa, int64_t stride,
                                                                   __half* __restrict__ coef16, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t tile = i >> 6, lane = i & 63u;
    if (half) {
        const float* rec = tiled + (size_t)tile * kPrmTileF16;
        soa[0 * stride + i] = rec[lane]; soa[1 * stride + i] = rec[64 + lane]; soa[2 * stride + i] = rec[128 + lane];
        soa[10 * stride + i] = rec[192 + lane];
        const __half* hrec = reinterpret_cast<const __half*>(rec + 256);
#pragma unroll
        for (int f = 0; f < 7; ++f) {
            const __half c = hrec[f * 64 + lane];
            coef16[f * stride + i] = c;
            soa[(3 + f) * stride + i] = __half2float(c);          // (the fp32 rows then hold what the kernels use)
        }
    } else {
        const float* rec = tiled + (size_t)tile * kPrmTileF32;
#pragma unroll
        for (int f = 0; f < 11; ++f) soa[f * stride + i] = rec[f * 64 + lane];
    }
}

// generic field-group repack between plain SoA ([F] pointers) and tiled, either direction
struct RepackArgs { float* soa[24]; float* tiled; uint32_t tile_stride; int fields; int to_tiled; uint32_t n; };
__global__ void __launch_bounds__(kBlock) repack_kernel(const RepackArgs a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t t = (i >> 6) * a.tile_stride + (i & 63u);
    for (int f = 0; f < a.fields; ++f) {
        if (a.to_tiled) a.tiled[t + f * 64] = a.soa[f][i];
        else a.soa[f][i] = a.tiled[t + f * 64];
    }
}

// simulator tensors (array-of-structs) -> tiled state, through LDS (same staging as the AoS wrench)
struct PackArgs { const float* pos; const float* quat; const float* vel; int quat_xyzw; float* st; uint32_t st_stride; uint32_t n; };
__global__ void __launch_bounds__(kBlock) pack_state_aos_kernel(const PackArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[kBlock * 9];
    const int t = threadIdx.x;
    const uint32_t block0 = blockIdx.x * kBlock;
    const uint32_t left = a.n - block0;
    if (left >= (uint32_t)kBlock) {
        const float4* p4 = reinterpret_cast<const float4*>(a.pos + (size_t)block0 * 3);
        const float4* v4 = reinterpret_cast<const float4*>(a.vel + (size_t)block0 * 6);
        if (t < kBlock * 3 / 4) reinterpret_cast<float4*>(lds + kBlock * 6)[t] = p4[t];
        reinterpret_cast<float4*>(lds)[t] = v4[t];
        if (t < kBlock * 6 / 4 - kBlock) reinterpret_cast<float4*>(lds)[t + kBlock] = v4[t + kBlock];
    } else {
        for (uint32_t k = t; k < left * 3; k += kBlock) lds[kBlock * 6 + k] = a.pos[(size_t)block0 * 3 + k];
        for (uint32_t k = t; k < left * 6; k += kBlock) lds[k] = a.vel[(size_t)block0 * 6 + k];
    }
    __syncthreads();
    const uint32_t i = block0 + t;
    if (i >= a.n) return;
    const float4 q = reinterpret_cast<const float4*>(a.quat)[i];
    float* rec = a.st + (size_t)(i >> 6) * a.st_stride + (i & 63u);
    rec[0 * 64] = lds[kBlock * 6 + 3 * t]; rec[1 * 64] = lds[kBlock * 6 + 3 * t + 1]; rec[2 * 64] = lds[kBlock * 6 + 3 * t + 2];
    if (a.quat_xyzw) { rec[3 * 64] = q.x; rec[4 * 64] = q.y; rec[5 * 64] = q.z; rec[6 * 64] = q.w; }
    else             { rec[3 * 64] = q.y; rec[4 * 64] = q.z; rec[5 * 64] = q.w; rec[6 * 64] = q.x; }
#pragma unroll
    for (int f = 0; f < 6; ++f) rec[(7 + f) * 64] = lds[6 * t + f];
}

// tiled wrench -> forces (n,3), torques (n,3), through LDS for whole-line stores
struct UnpackArgs { const float* w; uint32_t w_stride; float* force; float* torque; uint32_t n; };
__global__ void __launch_bounds__(kBlock) unpack_wrench_aos_kernel(const UnpackArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[kBlock * 6];
    const int t = threadIdx.x;
    const uint32_t block0 = blockIdx.x * kBlock;
    const uint32_t i = block0 + t;
    const uint32_t left = a.n - block0;
    if (i < a.n) {
        const float* rec = a.w + (size_t)(i >> 6) * a.w_stride + (i & 63u);
        lds[3 * t] = rec[0]; lds[3 * t + 1] = rec[64]; lds[3 * t + 2] = rec[128];
        lds[kBlock * 3 + 3 * t] = rec[192]; lds[kBlock * 3 + 3 * t + 1] = rec[256]; lds[kBlock * 3 + 3 * t + 2] = rec[320];
    }
    __syncthreads();
    if (left >= (uint32_t)kBlock) {
        if (t < kBlock * 3 / 4) {
            reinterpret_cast<float4*>(a.force + (size_t)block0 * 3)[t] = reinterpret_cast<const float4*>(lds)[t];
            reinterpret_cast<float4*>(a.torque + (size_t)block0 * 3)[t] = reinterpret_cast<const float4*>(lds + kBlock * 3)[t];
        }
    } else {
        for (uint32_t k = t; k < left * 3; k += kBlock) {
            a.force[(size_t)block0 * 3 + k] = lds[k];
            a.torque[(size_t)block0 * 3 + k] = lds[kBlock * 3 + k];
        }
    }
}

// --------------------------------------------------------------------------
// fused wrench on the simulator's array-of-structs tensors (hydro_step_wrench_aos): positions (n,3), orientations
// (n,4) wxyz or xyzw, velocities (n,6) in; forces (n,3), torques (n,3) out; previous velocity and parameters are the
// engine's tiled records.  168 B per body-step, all of it real traffic.
//
// Every lane reads ITS body's rows straight into registers - 12 B of position (global_load_dwordx3), 16 B of
// orientation (dwordx4), 24 B of velocity (dwordx4 + dwordx2) - and writes its force and torque rows as dwordx3.  A
// wave-instruction covers one contiguous 768-B / 1 024-B / 1 536-B run, so whole lines are consumed and the
// transposition costs nothing: gfx950 takes 4-byte-aligned wide accesses (unaligned access mode is on under HSA).
// Measured against the LDS-staged form below (whole 16-byte chunks per wave into a wave-private LDS slice, rows picked
// up with conflict-free strides, three wavefront fences): 30.3 vs 34.0 us at 1 M bodies, 111.6 vs 113.7 us at 4 M,
// identical bits; 91 % / 100 % of a memory-only probe of the same traffic (scripts/probes.py).
// --------------------------------------------------------------------------
template <bool NT, typename V>
__device__ __forceinline__ void stg_aos(V* p, V v) { stg_nt<NT>(p, v); }
typedef float f3_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef float f4_a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef float f2_a8 __attribute__((ext_vector_type(2), aligned(8)));
typedef float f4_a16 __attribute__((ext_vector_type(4), aligned(16)));
// (one function per type: a template parameter would drop the typedef's alignment and let the compiler assume 16)
#define HYDRO_WIDE_ACCESS(T, BYTES)                                                                                       \
    template <bool NT> __device__ __forceinline__ T ld_##T(const void* base, uint32_t byte_off)                              \
    { const T* q = reinterpret_cast<const T*>(static_cast<const char*>(base) + byte_off); if constexpr (NT) return __builtin_nontemporal_load(q); else return *q; } \
    template <bool NT> __device__ __forceinline__ void st_##T(void* base, uint32_t byte_off, T v)                            \
    { T* q = reinterpret_cast<T*>(static_cast<char*>(base) + byte_off);                                                      \
      if constexpr (NT) __builtin_nontemporal_store(v, q); else *q = v; }
HYDRO_WIDE_ACCESS(f3_a4, 12)
HYDRO_WIDE_ACCESS(f4_a8, 16)
HYDRO_WIDE_ACCESS(f2_a8, 8)
HYDRO_WIDE_ACCESS(f4_a16, 16)
#undef HYDRO_WIDE_ACCESS

template <bool HALF, bool NT, bool WARP>
__global__ void __launch_bounds__(kBlock) wrench_aos_direct_kernel(const float* k_pos, const float* k_quat, const float* k_vel, float* k_force, float* k_torque,
                                                                  float* k_pv, const float* k_prm, int quat_xyzw, uint32_t n,      // 16 dwords: preloaded
                                                                  int warp, double rho, double g, double inv_dt)
{
    // quat_xyzw: 0 = the simulator's order w,x,y,z, 1 = the kernels' x,y,z,w.  k_pv, k_prm: the engine's tiled previous velocity
    // (read, then updated) and parameter records.
    // (wave-uniform tile: the bases of the tile's rows and records are scalar adds, see load_tile_records)
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const size_t first = (size_t)tile * 64u;
    const float* t_pos = k_pos + first * 3; const float* t_quat = k_quat + first * 4; const float* t_vel = k_vel + first * 6;
    float s[HYDRO_STATE_FIELDS], pv[HYDRO_PREV_FIELDS], d[3], c[7], mass;
    // The simulator's rows are read with TEMPORAL loads whatever the size: the simulator has just written them, so they
    // are the one input that can still be in L2 / the Infinity Cache (the engine's own records and the outputs stream).
    // Measured (A/B against a build whose row loads stream too): equal when nothing can be resident (8 rotating sets
    // of 1 M bodies: 29.84 vs 29.96 us; 4 M: 112.2 vs 112.3), 12 % faster when the rows are (4 sets: 26.5 vs 30.2 us) -
    // which is also why bench.py rotates EIGHT sets for this entry: its figure must be an HBM rate.
    constexpr bool RNT = false;
    const f3_a4 p = ld_f3_a4<RNT>(t_pos, lane * 12u);
    const f4_a16 q = ld_f4_a16<RNT>(t_quat, lane * 16u);
    const f4_a8 v0 = ld_f4_a8<RNT>(t_vel, lane * 24u);
    const f2_a8 v1 = ld_f2_a8<RNT>(t_vel, lane * 24u + 16u);
    s[0] = p.x; s[1] = p.y; s[2] = p.z;
    if (quat_xyzw) { s[3] = q.x; s[4] = q.y; s[5] = q.z; s[6] = q.w; }
    else           { s[3] = q.y; s[4] = q.z; s[5] = q.w; s[6] = q.x; }   // wxyz -> xyzw (hydrodynamics_behavior.py:194)
    s[7] = v0.x; s[8] = v0.y; s[9] = v0.z; s[10] = v0.w; s[11] = v1.x; s[12] = v1.y;
    float* t_pv = k_pv + (size_t)tile * (HYDRO_PREV_FIELDS * HYDRO_TILE);
#pragma unroll
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) pv[f] = ldg<NT>(at<float>(t_pv, lane4, f * 256u));
    load_param_record<HALF, NT>(k_prm, tile, lane4, d, c, mass);
    const hydro::Wrench w = body_wrench(s, pv, d, c, mass, rho, g, inv_dt, WARP);
#pragma unroll
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) stg_aos<NT>(at<float>(t_pv, lane4, f * 256u), s[7 + f]);
    f3_a4 fo, to;
    fo.x = w.fx; fo.y = w.fy; fo.z = w.fz; to.x = w.tx; to.y = w.ty; to.z = w.tz;
    st_f3_a4<NT>(k_force + first * 3, lane * 12u, fo);
    st_f3_a4<NT>(k_torque + first * 3, lane * 12u, to);
}

// --------------------------------------------------------------------------
// component mode (compatibility / debug surface, not a benchmark mode)
// --------------------------------------------------------------------------
struct CompArgs {
    const float* st[HYDRO_STATE_FIELDS];
    const float* acc[HYDRO_PREV_FIELDS];
    const float* dims[3];
    const void* coef[7];
    float* out[HYDRO_COMP_FIELDS];
    float* ratio;
    double rho, g;
    int warp;
    int64_t n;
};

template <bool HALF>
__global__ void __launch_bounds__(kBlock) components_kernel(const CompArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    hydro::BodyIn b;
    b.px = a.st[0][i]; b.py = a.st[1][i]; b.pz = a.st[2][i];
    b.qx = a.st[3][i]; b.qy = a.st[4][i]; b.qz = a.st[5][i]; b.qw = a.st[6][i];
    b.vx = a.st[7][i]; b.vy = a.st[8][i]; b.vz = a.st[9][i];
    b.wx = a.st[10][i]; b.wy = a.st[11][i]; b.wz = a.st[12][i];
    b.dimx = a.dims[0][i]; b.dimy = a.dims[1][i]; b.dimz = a.dims[2][i];
    b.cd_lin = load_coef1<HALF>(a.coef[0], i); b.cd_ang = load_coef1<HALF>(a.coef[1], i);
    b.damp_lin = load_coef1<HALF>(a.coef[2], i); b.damp_ang = load_coef1<HALF>(a.coef[3], i);
    b.lift = load_coef1<HALF>(a.coef[4], i); b.am_lin = load_coef1<HALF>(a.coef[5], i);
    b.am_ang = load_coef1<HALF>(a.coef[6], i);
    const hydro::Body o = hydro::solve_body(b, a.acc[0][i], a.acc[1][i], a.acc[2][i], a.acc[3][i], a.acc[4][i], a.acc[5][i], 1.0,
                                            a.rho, a.g, a.warp != 0);
    const hydro::Components c = hydro::round_components(o, b, a.warp != 0);
    // reference order: buoyancy F, drag F, lift F, drag T, added-mass F, added-mass T, cob, cop (world space; zeros
    // when dry - Numba semantics, numba_hydrodynamics.py:277-279)
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int x = 0; x < 3; ++x) a.out[3 * k + x][i] = c.v[k][x];
    if (a.ratio) a.ratio[i] = c.ratio;
}

// component mode on the calculator's own argument layout: six (n,3)/(n,4) tensors in, eight (n,3)
// tensors out (+ ratio) - ONE launch per calculate_hydrodynamic_forces call, where the reference's
// Warp wrapper needs six assign copies and a graph launch (warp_hydrodynamics_wrapper.py:85-120).
struct CompAosArgs {
    const float* pos; const float* quat_xyzw; const float* lin_vel; const float* ang_vel;
    const float* lin_acc; const float* ang_acc;                 // (n,3) except quat (n,4)
    const float* prm;                                            // engine-owned tiled parameter record
    float* out[8];                                               // eight (n,3) tensors, reference order
    float* ratio;
    double rho, g;
    int warp;
    uint32_t n;
};

template <bool HALF>
__global__ void __launch_bounds__(kBlock) components_aos_kernel(const CompAosArgs a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    hydro::BodyIn b;
    b.px = a.pos[3 * i]; b.py = a.pos[3 * i + 1]; b.pz = a.pos[3 * i + 2];
    // component-wise: a one-row slice handed over by a caller may start at any 4-byte offset
    b.qx = a.quat_xyzw[4 * i]; b.qy = a.quat_xyzw[4 * i + 1]; b.qz = a.quat_xyzw[4 * i + 2]; b.qw = a.quat_xyzw[4 * i + 3];
    b.vx = a.lin_vel[3 * i]; b.vy = a.lin_vel[3 * i + 1]; b.vz = a.lin_vel[3 * i + 2];
    b.wx = a.ang_vel[3 * i]; b.wy = a.ang_vel[3 * i + 1]; b.wz = a.ang_vel[3 * i + 2];
    const uint32_t tile = i >> 6, lane = i & 63u;
    float c[7];
    if constexpr (HALF) {
        const uint32_t qo = __umul24(tile, kPrmTileF16 * 4u) + lane * 4u;
        b.dimx = *at<float>(a.prm, qo); b.dimy = *at<float>(a.prm, qo, 256u); b.dimz = *at<float>(a.prm, qo, 512u);
        const uint32_t ho = __umul24(tile, kPrmTileF16 * 4u) + 1024u + lane * 2u;
#pragma unroll
        for (int f = 0; f < 7; ++f) c[f] = half_bits_to_float(*at<unsigned short>(a.prm, ho, f * 128u));
    } else {
        const uint32_t qo = __umul24(tile, kPrmTileF32 * 4u) + lane * 4u;
        b.dimx = *at<float>(a.prm, qo); b.dimy = *at<float>(a.prm, qo, 256u); b.dimz = *at<float>(a.prm, qo, 512u);
#pragma unroll
        for (int f = 0; f < 7; ++f) c[f] = *at<float>(a.prm, qo + (3 + f) * 256u);
    }
    b.cd_lin = c[0]; b.cd_ang = c[1]; b.damp_lin = c[2]; b.damp_ang = c[3]; b.lift = c[4]; b.am_lin = c[5]; b.am_ang = c[6];
    const hydro::Body o = hydro::solve_body(b, a.lin_acc[3 * i], a.lin_acc[3 * i + 1], a.lin_acc[3 * i + 2],
                                            a.ang_acc[3 * i], a.ang_acc[3 * i + 1], a.ang_acc[3 * i + 2], 1.0, a.rho, a.g, a.warp != 0);
    const hydro::Components r = hydro::round_components(o, b, a.warp != 0);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        a.out[k][3 * i] = r.v[k][0]; a.out[k][3 * i + 1] = r.v[k][1]; a.out[k][3 * i + 2] = r.v[k][2];
    }
    if (a.ratio) a.ratio[i] = r.ratio;
}

// --------------------------------------------------------------------------
// kinetic energy, stand-alone (hydro_kinetic_energy[_tiled]): one pass over 56 B per body with the rotational term (40
// of the 52 state bytes + dimensions and mass), 20 B without - a pure streaming kernel, HBM-bound, in the shape of the
// in-kernel sampling: one body per lane, every load issued before the first use, one group per block.  (Measured against
// a wavefront per group - four tiles per lane, 44 loads in flight, no LDS: 12.1 vs 11.05 us at 1 M bodies and 37.1 vs
// 35.6 us at 4 M before the final sum; the memory-only probe of the same bytes takes 9.9 / 35.3 us.  Many short waves
// overlap one wave's arithmetic with the others' loads; few long ones do all their arithmetic after their data.)
// State from plain SoA field pointers or from a tiled buffer (one address rule, see IntArgs); dimensions and mass from the
// engine's tiled parameter record.
// --------------------------------------------------------------------------
struct KeArgs {
    const float* st[HYDRO_STATE_FIELDS];   // plain SoA field pointers, or tiled base + f*64
    uint32_t st_stride, shift, mask;
    const float* prm;                      // engine-owned tiled parameter record
    uint32_t prm_tile_floats, mass_field;  // 704 / 10 (fp32 record) or 480 / 3 (fp16-coefficient record)
    double* partials; uint32_t partial_stride;
    double* out;
    uint32_t n;
};

template <bool ROT>
__global__ void __launch_bounds__(kBlock) ke_kernel(const KeArgs a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    double lin = 0.0, rot = 0.0;
    if (i < a.n) {
        // state: field base pointers in SGPRs + one 32-bit byte offset (i < 2^30; tiled buffers < 4 GiB);
        // parameter record: one 64-bit address, field offsets in the instruction
        const uint32_t o = ((i >> a.shift) * a.st_stride + (i & a.mask)) * 4u;
        const float* pr = a.prm + (size_t)(i >> 6) * a.prm_tile_floats + (i & 63u);
        const float m = __builtin_nontemporal_load(pr + a.mass_field * 64u);
        float v[3], q[4] = {0.f, 0.f, 0.f, 1.f}, w[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = ldg<true>(at<float>(a.st[7 + k], o));
        if constexpr (ROT) {
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = ldg<true>(at<float>(a.st[3 + k], o));
#pragma unroll
            for (int k = 0; k < 3; ++k) { w[k] = ldg<true>(at<float>(a.st[10 + k], o)); d[k] = __builtin_nontemporal_load(pr + k * 64); }
        }
        hydro::kinetic_energy(q[0], q[1], q[2], q[3], v[0], v[1], v[2], w[0], w[1], w[2], d[0], d[1], d[2], m, ROT, lin, rot);
    }
    ke_block_reduce(lin, rot, a.partials, a.partial_stride, a.out);
}

// --------------------------------------------------------------------------
// explicit rigid-body step (stands in for PhysX in closed-loop runs)
// --------------------------------------------------------------------------
// One address rule covers both layouts: field k of body i is at  p[k] + (i >> shift) * stride + (i & mask)
// plain SoA: p[k] = field pointer, shift = 31 (tile index 0), mask = ~0u;  tiled: p[k] = base + k*64, shift 6, mask 63.
struct IntArgs {
    const float* si[HYDRO_STATE_FIELDS]; uint32_t si_stride;
    const float* w[HYDRO_WRENCH_FIELDS]; uint32_t w_stride;
    float* so[HYDRO_STATE_FIELDS];       uint32_t so_stride;
    const float* prm;                    // engine-owned tiled parameter record (dimensions, mass)
    uint32_t prm_tile_floats, mass_field;  // 704 / 10 (fp32 record) or 480 / 3 (fp16-coefficient record)
    uint32_t shift, mask;
    float g, dt;
    uint32_t n;
};

// semi-implicit Euler with gravity and box inertia for one body: s[13], wrench f[6] -> o[13]
//
// IMPLICIT (fused step only): the drag part of the wrench, k_lin * v and k_ang * w with k <= 0, is
// taken at the NEW velocity (coefficients frozen at the old state):
//     m (v' - v)/dt = (F - k_lin v) + k_lin v' + m g     =>   v' = (m v + dt (F - k_lin v + m g)) / (m - dt k_lin)
// and likewise per principal axis for the angular part.  Unconditionally stable in the drag terms -
// the explicit form needs |k| dt / m < 2, which the 0.45 kg SILVER2 links at 120 Hz violate (5.5).
// 1/x and 1/sqrt(x) in fp32: the hardware seed (1 ulp) and one Newton step (~0.5 ulp) - 3 and 4 instructions where the
// IEEE-exact division and sqrt + division expand to ~10 and ~20.  The integrator stands in for PhysX in closed-loop runs
// (SURVEY.md 8f row 2): it has no reference to be bit-exact with.
__device__ __forceinline__ float rcp_nr(float x)
{
    const float r = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
}
__device__ __forceinline__ float rsqrt_nr(float x)
{
    const float r = __builtin_amdgcn_rsqf(x);
    return __builtin_fmaf(__builtin_fmaf(-x * r, r, 1.0f), 0.5f * r, r);
}

// The fp32 rotation matrix of a quaternion as given (non-unit included), body -> world: the one form the integrator and the
// body-frame applied wrench turn vectors with.
struct Rotation { float r00, r01, r02, r10, r11, r12, r20, r21, r22; };
__device__ __forceinline__ Rotation rotation_of(float qx, float qy, float qz, float qw)
{
    const float x2 = qx + qx, y2 = qy + qy, z2 = qz + qz;
    const float xx = qx * x2, xy = qx * y2, xz = qx * z2, yy = qy * y2, yz = qy * z2, zz = qz * z2;
    const float sx = qw * x2, sy = qw * y2, sz = qw * z2;
    return {1.0f - (yy + zz), xy - sz, xz + sy,
            xy + sz, 1.0f - (xx + zz), yz - sx,
            xz - sy, yz + sx, 1.0f - (xx + yy)};
}

template <bool IMPLICIT>
__device__ __forceinline__ void integrate_body(const float (&s)[HYDRO_STATE_FIELDS], const float (&f)[HYDRO_WRENCH_FIELDS],
                                               float m, float dx, float dy, float dz, float g, float dt,
                                               float k_lin, float k_ang, float (&o)[HYDRO_STATE_FIELDS])
{
    const float inv_m = rcp_nr(m);
    float vx, vy, vz;
    if constexpr (IMPLICIT) {
        const float den = rcp_nr(m - dt * k_lin);
        vx = (m * s[7] + dt * (f[0] - k_lin * s[7])) * den;
        vy = (m * s[8] + dt * (f[1] - k_lin * s[8])) * den;
        vz = (m * s[9] + dt * (f[2] - k_lin * s[9] - m * g)) * den;
    } else {
        // linear: semi-implicit Euler, gravity along -z
        vx = s[7] + dt * (f[0] * inv_m); vy = s[8] + dt * (f[1] * inv_m); vz = s[9] + dt * (f[2] * inv_m - g);
    }
    const float px = s[0] + dt * vx, py = s[1] + dt * vy, pz = s[2] + dt * vz;
    // angular, body frame: I w' = tau_b - w_b x (I w_b), box inertia
    const float qx = s[3], qy = s[4], qz = s[5], qw = s[6];
    const auto [r00, r01, r02, r10, r11, r12, r20, r21, r22] = rotation_of(qx, qy, qz, qw);
    const float k = m * (1.0f / 12.0f);
    const float ix = k * (dy * dy + dz * dz), iy = k * (dx * dx + dz * dz), iz = k * (dx * dx + dy * dy);
    const float wbx = r00 * s[10] + r10 * s[11] + r20 * s[12];
    const float wby = r01 * s[10] + r11 * s[11] + r21 * s[12];
    const float wbz = r02 * s[10] + r12 * s[11] + r22 * s[12];
    const float tbx = r00 * f[3] + r10 * f[4] + r20 * f[5];
    const float tby = r01 * f[3] + r11 * f[4] + r21 * f[5];
    const float tbz = r02 * f[3] + r12 * f[4] + r22 * f[5];
    float nbx, nby, nbz;
    if constexpr (IMPLICIT) {
        nbx = (ix * wbx + dt * (tbx - k_ang * wbx - (wby * (iz * wbz) - wbz * (iy * wby)))) * rcp_nr(ix - dt * k_ang);
        nby = (iy * wby + dt * (tby - k_ang * wby - (wbz * (ix * wbx) - wbx * (iz * wbz)))) * rcp_nr(iy - dt * k_ang);
        nbz = (iz * wbz + dt * (tbz - k_ang * wbz - (wbx * (iy * wby) - wby * (ix * wbx)))) * rcp_nr(iz - dt * k_ang);
    } else {
        nbx = wbx + dt * (tbx - (wby * (iz * wbz) - wbz * (iy * wby))) * rcp_nr(ix);
        nby = wby + dt * (tby - (wbz * (ix * wbx) - wbx * (iz * wbz))) * rcp_nr(iy);
        nbz = wbz + dt * (tbz - (wbx * (iy * wby) - wby * (ix * wbx))) * rcp_nr(iz);
    }
    const float wx = r00 * nbx + r01 * nby + r02 * nbz;
    const float wy = r10 * nbx + r11 * nby + r12 * nbz;
    const float wz = r20 * nbx + r21 * nby + r22 * nbz;
    // q' = normalise(q + dt/2 * (w,0) (x) q)
    const float h = 0.5f * dt;
    float nqx = qx + h * (wx * qw + wy * qz - wz * qy);
    float nqy = qy + h * (wy * qw + wz * qx - wx * qz);
    float nqz = qz + h * (wz * qw + wx * qy - wy * qx);
    float nqw = qw - h * (wx * qx + wy * qy + wz * qz);
    const float inv_n = rsqrt_nr(nqx * nqx + nqy * nqy + nqz * nqz + nqw * nqw);
    o[0] = px; o[1] = py; o[2] = pz;
    o[3] = nqx * inv_n; o[4] = nqy * inv_n; o[5] = nqz * inv_n; o[6] = nqw * inv_n;
    o[7] = vx; o[8] = vy; o[9] = vz;
    o[10] = wx; o[11] = wy; o[12] = wz;
}

__global__ void __launch_bounds__(kBlock) integrate_kernel(const IntArgs a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t hi = i >> a.shift, lo = i & a.mask;
    const uint32_t oi = hi * a.si_stride + lo, ow = hi * a.w_stride + lo, oo = hi * a.so_stride + lo;
    float s[HYDRO_STATE_FIELDS], f[HYDRO_WRENCH_FIELDS], o[HYDRO_STATE_FIELDS];
#pragma unroll
    for (int k = 0; k < HYDRO_STATE_FIELDS; ++k) s[k] = a.si[k][oi];
#pragma unroll
    for (int k = 0; k < HYDRO_WRENCH_FIELDS; ++k) f[k] = a.w[k][ow];
    const float* q = a.prm + (size_t)(i >> 6) * a.prm_tile_floats + (i & 63u);
    integrate_body<false>(s, f, q[a.mass_field * 64u], q[0], q[64], q[128], a.g, a.dt, 0.0f, 0.0f, o);
#pragma unroll
    for (int k = 0; k < HYDRO_STATE_FIELDS; ++k) a.so[k][oo] = o[k];
}

// --------------------------------------------------------------------------
// fused closed-loop step on tiled buffers: wrench + integrator in one pass.  The state is read
// once, the wrench never goes through HBM (unless asked for): 120 B read + 52 B written per
// body-step instead of 280 B for the two separate kernels.  state_out may alias the buffer the
// previous velocity is read from (ping-pong): each lane reads its own fields before writing them.
// --------------------------------------------------------------------------
// KE = true: also samples the kinetic energy of the state it WRITES (the state after this step), see wrench_tiled_kernel.
// k_out == nullptr: the wrench is not stored.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) step_fused_tiled_kernel(const float* k_st, const float* k_pv, const float* k_prm, float* k_so, float* k_out,
                                                                 uint32_t st_stride, uint32_t pv_stride, uint32_t so_stride, uint32_t out_stride,
                                                                 uint32_t n, int warp, float dt, double rho, double g, double inv_dt,
                                                                 double* ke_partials, uint32_t ke_stride, int ke_rotational, double* ke_out)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;      // (wave-uniform, see load_tile_records)
    const bool live = tile * 64u + lane < n;
    if constexpr (!KE) {
        if (!live) return;
    }
    double ke_lin = 0.0, ke_rot = 0.0;
    if (!KE || live) {
        float s[HYDRO_STATE_FIELDS], pv[HYDRO_PREV_FIELDS], d[3], c[7], mass, f6[HYDRO_WRENCH_FIELDS], o[HYDRO_STATE_FIELDS];
        load_tile_records<HALF, NT>(k_st + (size_t)tile * st_stride, k_pv + (size_t)tile * pv_stride, k_prm, tile, lane4, s, pv, d, c, mass);
        const hydro::Wrench w = body_wrench(s, pv, d, c, mass, rho, g, inv_dt, WARP);
        wrench_fields(w, f6);
        integrate_body<IMPLICIT>(s, f6, mass, d[0], d[1], d[2], g, dt, w.k_lin, w.k_ang, o);     // (k_lin, k_ang: the implicit form only)
        if constexpr (KE)
            hydro::kinetic_energy(o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10], o[11], o[12], d[0], d[1], d[2], mass,
                                  ke_rotational != 0, ke_lin, ke_rot);
        store_record<HYDRO_STATE_FIELDS, NT>(k_so + (size_t)tile * so_stride, lane4, o);
        if (k_out) store_record<HYDRO_WRENCH_FIELDS, NT>(k_out + (size_t)tile * out_stride, lane4, f6);
    }
    if constexpr (KE) ke_block_reduce(ke_lin, ke_rot, ke_partials, ke_stride, ke_out);
}

// One closed-loop step of a body held in registers - the loop body of the two multi-step kernels below: the wrench of
// (s, pv), the integrator, then pv <- the velocity just used and s <- the new state.  f6 is the wrench that produced the new s.
// `app` is the applied-wrench policy: add(s, f6) between the (clamped) hydrodynamic wrench and the integrator.
// `sea` is the sea-state policy: view(k, s, pv) puts the state RELATIVE to the local water in front of body_wrench (depth below
// the local surface, velocity against the local water), restore(s, pv) brings the true one back behind it - everything
// after the wrench acts on the true state (see SeaView; NoSea does nothing, and the kernels without a sea are unchanged).
// `bed` is the seabed policy: add(s, d, mass, f6) behind app.add, before the integrator (see SeabedContact; NoBed does nothing).
// `moor` is the mooring policy: add(s, f6) behind bed.add, before the integrator (see MooringLine; NoMooring does nothing).
// `teth` is the tether policy: add(s, f6) behind moor.add, before the integrator (see TetherLine; NoTether does nothing).
template <bool IMPLICIT, bool WARP, typename Applied, typename Sea, typename Bed, typename Moor, typename Teth>
__device__ __forceinline__ void fused_step_in_registers(float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS], const float (&d)[3], const float (&c)[7], float mass,
                                                        double rho, double g, double inv_dt, float dt, float (&f6)[HYDRO_WRENCH_FIELDS], const Applied& app,
                                                        uint32_t k, const Sea& sea, const Bed& bed, const Moor& moor, const Teth& teth)
{
    sea.view(k, s, pv);
    const hydro::Wrench w = body_wrench(s, pv, d, c, mass, rho, g, inv_dt, WARP);
    sea.restore(s, pv);
    wrench_fields(w, f6);
    app.add(s, f6);
    bed.add(s, d, mass, f6);
    moor.add(s, f6);
    teth.add(s, f6);
    float o[HYDRO_STATE_FIELDS];
    integrate_body<IMPLICIT>(s, f6, mass, d[0], d[1], d[2], g, dt, w.k_lin, w.k_ang, o);
#pragma unroll
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) pv[f] = s[7 + f];
#pragma unroll
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) s[f] = o[f];
}

// --------------------------------------------------------------------------
// `steps` closed-loop steps in ONE pass: no term of the model couples two bodies, so a lane can carry its body through any
// number of steps in registers - state, previous velocity and the 11 parameters are read once, the state after the last
// step and the velocity of the step before it are written once.  Per body-step that is (120 + 76) / steps bytes instead
// of 172, and one launch instead of `steps`: the loop is bound by the arithmetic alone (section 6 of DESIGN.md).
// Same arithmetic, same order, hence the same bits as `steps` launches of step_fused_tiled_kernel.
// k_pvo may alias the velocity fields of the state this kernel READS (each lane reads its own fields first): the
// two-buffer ping-pong of the single-step entry then carries over unchanged.
// --------------------------------------------------------------------------
// The body of the three kernels below.  `rec` is the recorder policy: begin(tile, lane) once the records are loaded, then
// after_step(k, s, f6) behind every step with the state it produced and the wrench that produced it.  `app` is the
// applied-wrench policy: begin(tile, lane4) next to the record loads, then add(s, f6) inside every step (see AppliedWrench).
// `sea` is the sea-state policy: begin(lane4) next to the record loads, then view / restore around every step's wrench.
// `bed` is the seabed policy: add(s, d, mass, f6) inside every step; it carries scene constants only and has no begin.
// `moor` is the mooring policy: begin(tile, lane4) next to the record loads, then add(s, f6) inside every step, and end(d)
// behind the last step of a kernel that samples the kinetic energy (see MooringLine).
// `ext` is the extremes policy: begin(tile, lane4) next to the record loads, after_step(s, T) behind rec.after_step with the
// state the step produced and the tension moor.add formed in it, end(tile, lane4) in front of the final stores (see
// ExtremesTrack; NoExtremes does nothing).
// `teth` is the tether policy: begin(tile, lane4) next to the record loads, then add(s, f6) inside every step, behind moor.add
// (see TetherLine; NoTether does nothing).
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP, typename Recorder, typename Applied, typename Sea, typename Bed, typename Moor, typename Ext, typename Teth>
__device__ __forceinline__ void fused_multi_body(const float* k_st, const float* k_pv, const float* k_prm, float* k_so, float* k_pvo,
                                                 uint32_t st_stride, uint32_t pv_stride, uint32_t so_stride, uint32_t pvo_stride,
                                                 uint32_t n, uint32_t steps, float dt, double rho, double g, double inv_dt,
                                                 double* ke_partials, uint32_t ke_stride, int ke_rotational, double* ke_out, Recorder rec, Applied app, Sea sea, Bed bed, Moor moor, Ext ext, Teth teth)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;      // (wave-uniform, see load_tile_records)
    const bool live = tile * 64u + lane < n;
    if constexpr (!KE) {
        if (!live) return;
    }
    double ke_lin = 0.0, ke_rot = 0.0;
    if (!KE || live) {
        float s[HYDRO_STATE_FIELDS], pv[HYDRO_PREV_FIELDS], d[3], c[7], mass;
        load_tile_records<HALF, NT>(k_st + (size_t)tile * st_stride, k_pv + (size_t)tile * pv_stride, k_prm, tile, lane4, s, pv, d, c, mass);
        rec.begin(tile, lane);
        app.begin(tile, lane4);
        sea.begin(lane4);
        moor.begin(tile, lane4);
        ext.begin(tile, lane4);
        teth.begin(tile, lane4);
#pragma unroll 1
        for (uint32_t k = 0; k < steps; ++k) {
            float f6[HYDRO_WRENCH_FIELDS];
            fused_step_in_registers<IMPLICIT, WARP>(s, pv, d, c, mass, rho, g, inv_dt, dt, f6, app, k, sea, bed, moor, teth);
            rec.after_step(k, s, f6);
            ext.after_step(s, moor.tension());
        }
        if constexpr (KE) {
            moor.end(d);
            hydro::kinetic_energy(s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11], s[12], d[0], d[1], d[2], mass,
                                  ke_rotational != 0, ke_lin, ke_rot);
        }
        ext.end(tile, lane4);
        store_record<HYDRO_PREV_FIELDS, NT>(k_pvo + (size_t)tile * pvo_stride, lane4, pv);
        store_record<HYDRO_STATE_FIELDS, NT>(k_so + (size_t)tile * so_stride, lane4, s);
    }
    if constexpr (KE) ke_block_reduce(ke_lin, ke_rot, ke_partials, ke_stride, ke_out);
}

struct NoRecorder {
    __device__ __forceinline__ void begin(uint32_t, uint32_t) {}
    __device__ __forceinline__ void after_step(uint32_t, const float (&)[HYDRO_STATE_FIELDS], const float (&)[HYDRO_WRENCH_FIELDS]) {}
};
struct NoApplied {
    __device__ __forceinline__ void begin(uint32_t, uint32_t) {}
    __device__ __forceinline__ void add(const float (&)[HYDRO_STATE_FIELDS], float (&)[HYDRO_WRENCH_FIELDS]) const {}
};
struct NoSea {
    __device__ __forceinline__ void begin(uint32_t) {}
    __device__ __forceinline__ void view(uint32_t, float (&)[HYDRO_STATE_FIELDS], float (&)[HYDRO_PREV_FIELDS]) const {}
    __device__ __forceinline__ void restore(float (&)[HYDRO_STATE_FIELDS], float (&)[HYDRO_PREV_FIELDS]) const {}
};
struct NoBed {
    __device__ __forceinline__ void add(const float (&)[HYDRO_STATE_FIELDS], const float (&)[3], float, float (&)[HYDRO_WRENCH_FIELDS]) const {}
};
struct NoMooring {
    __device__ __forceinline__ void begin(uint32_t, uint32_t) {}
    __device__ __forceinline__ void end(float (&)[3]) const {}
    __device__ __forceinline__ void add(const float (&)[HYDRO_STATE_FIELDS], float (&)[HYDRO_WRENCH_FIELDS]) const {}
    __device__ __forceinline__ float tension() const { return 0.0f; }
};
struct NoExtremes {
    __device__ __forceinline__ void begin(uint32_t, uint32_t) {}
    __device__ __forceinline__ void after_step(const float (&)[HYDRO_STATE_FIELDS], float) const {}
    __device__ __forceinline__ void end(uint32_t, uint32_t) const {}
};
struct NoTether {
    __device__ __forceinline__ void begin(uint32_t, uint32_t) {}
    __device__ __forceinline__ void add(const float (&)[HYDRO_STATE_FIELDS], float (&)[HYDRO_WRENCH_FIELDS]) const {}
};

// --------------------------------------------------------------------------
// THE ARGUMENT GROUPS of the step_fused_multi_*_tiled_kernel family, each spelled ONCE: HYDRO_<GROUP>_PARAMS is the group as
// kernel parameters, HYDRO_<GROUP>_ARGS the same names as arguments.  A kernel's signature is a run of groups (every family
// takes its predecessor's and one more) and its body one fused_multi_body call; a group's policy is built from its ARGS by an
// inline factory that stands behind the policy's struct (log_recorder / optional_recorder, pose_hold / optional_pose_hold, ...)
// and takes the group's PARAMS as its own parameters.
// Macros and not by-value structs: a struct per group, laid out so that every kernarg offset stays where it is, still
// changed every instantiation it was tried on (other SGPR allocation, regrouped s_load_dwordx2/x4 from the kernarg
// segment, other mangled names), and these kernels stand at 163-167 of 168 VGPRs with the first 16 kernarg dwords preloaded
// (BASE's: tests/test_recorder.py).  The preprocessor leaves the flattened signatures, hence the code, as they were:
// scripts/asm_symbols.py shows every kernel of the file identical (section 26 of DESIGN.md).
// --------------------------------------------------------------------------
#define HYDRO_BASE_PARAMS const float* k_st, const float* k_pv, const float* k_prm, float* k_so, float* k_pvo,                   \
                          uint32_t st_stride, uint32_t pv_stride, uint32_t so_stride, uint32_t pvo_stride,                       \
                          uint32_t n, uint32_t steps, float dt, double rho, double g, double inv_dt,                             \
                          double* ke_partials, uint32_t ke_stride, int ke_rotational, double* ke_out
#define HYDRO_BASE_ARGS k_st, k_pv, k_prm, k_so, k_pvo, st_stride, pv_stride, so_stride, pvo_stride, n, steps, dt, rho, g, inv_dt, \
                        ke_partials, ke_stride, ke_rotational, ke_out
#define HYDRO_REC_PARAMS const uint64_t* w_mask, const uint32_t* w_first, float* log, uint32_t log_stride,                        \
                         uint32_t fields, uint32_t every, uint32_t phase, uint32_t row0
#define HYDRO_REC_ARGS w_mask, w_first, log, log_stride, fields, every, phase, row0
#define HYDRO_APP_PARAMS const float* applied, uint32_t applied_stride, int body_frame
#define HYDRO_APP_ARGS applied, applied_stride, body_frame
#define HYDRO_CTL_PARAMS const float* control, uint32_t control_stride
#define HYDRO_CTL_ARGS control, control_stride
#define HYDRO_SEA_PARAMS const void* sea_table, uint32_t sea_waves, int64_t step0, double sea_dt
#define HYDRO_SEA_ARGS sea_table, sea_waves, step0, sea_dt
#define HYDRO_BED_PARAMS float bed_z, float bed_stiffness, float bed_damping, float bed_friction, float bed_slip_speed, float bed_friction_rate
#define HYDRO_BED_ARGS bed_z, bed_stiffness, bed_damping, bed_friction, bed_slip_speed, bed_friction_rate
#define HYDRO_OPT_BED_PARAMS HYDRO_BED_PARAMS, int bed_present                   // (the families behind _bed: the bed is optional)
#define HYDRO_OPT_BED_ARGS HYDRO_BED_ARGS, bed_present
#define HYDRO_MOOR_PARAMS const float* mooring, uint32_t mooring_stride
#define HYDRO_MOOR_ARGS mooring, mooring_stride
#define HYDRO_EXT_PARAMS float* extremes, uint32_t extremes_stride
#define HYDRO_EXT_ARGS extremes, extremes_stride
#define HYDRO_TETH_PARAMS const float* tether, uint32_t tether_stride
#define HYDRO_TETH_ARGS tether, tether_stride
#define HYDRO_NET_PARAMS HYDRO_TETH_PARAMS, uint32_t layers                      // (the families behind _teth: the record is a net)
#define HYDRO_NET_ARGS HYDRO_TETH_ARGS, layers
#define HYDRO_PEAK_PARAMS float* peaks, uint32_t peaks_stride
#define HYDRO_PEAK_ARGS peaks, peaks_stride
#define HYDRO_SPREAD_PARAMS HYDRO_MOOR_PARAMS, uint32_t mooring_layers           // (the family behind _peak: the mooring record is a spread)
#define HYDRO_SPREAD_ARGS HYDRO_MOOR_ARGS, mooring_layers
// The three tether families share everything in front of the tether: the groups up to the extremes, every one optional.
#define HYDRO_UP_TO_EXT_PARAMS HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS, HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS,      \
                               HYDRO_MOOR_PARAMS, HYDRO_EXT_PARAMS
#define HYDRO_UP_TO_EXT_OPTIONAL HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),             \
                                 optional_sea_view(HYDRO_SEA_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS), optional_mooring_line(HYDRO_MOOR_ARGS), \
                                 optional_extremes_track(HYDRO_EXT_ARGS)
// What the policies that park in LDS ask for (see PoseHold): 3 waves per SIMD, named once like HYDRO_TILED_OCC_ATTR.
#define HYDRO_MULTI_OCC_ATTR __attribute__((amdgpu_waves_per_eu(3)))

// --------------------------------------------------------------------------
// The TRAJECTORY RECORDER in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_rec): the states between the
// first and the last step of a launch exist in registers only, so the bodies on the engine's watch list are written to a
// device log from inside the loop.  Everything the recorder decides on is wave-uniform:
//   w_mask / w_first : the watch tables of hydro_set_watch (hydro_watch.h), one entry per tile = per wavefront: which lanes
//                      are watched and the log column of the first of them; two scalar loads per wave and LAUNCH.  A
//                      watched lane's column is w_first[tile] + popcount(w_mask[tile] & lanes below it) - v_mbcnt
//   cadence          : a sample is due after local step k (1-based) when k >= phase and (k - phase) % every == 0, at row
//                      row0 + (k - phase) / every; kept as a running pair (next due step, its row), so the loop pays one
//                      scalar compare per step and no division.  A wave that watches nobody has no due step at all
//   log              : log[(row * fields + f) * log_stride + column], fields = 13 (state) or 19 (+ the wrench that produced
//                      it; a run-time flag: the instantiations are those of the plain kernel).  Ordinary vector stores, from
//                      the watched lanes only; the host has checked that every row of the launch exists
// The recorder reads registers and nothing it computes feeds back: state, prev_out and kinetic-energy bits are those of
// step_fused_multi_tiled_kernel.
// --------------------------------------------------------------------------
struct LogRecorder {
    const uint64_t* w_mask; const uint32_t* w_first; float* log; uint32_t log_stride, fields, every, phase, row0;
    bool watched; uint32_t column, due, row;
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane)
    {
        const uint64_t m = w_mask[tile];
        watched = ((m >> lane) & 1u) != 0;                  // (the host has checked that every watched body is < n: a live lane)
        column = w_first[tile] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        due = m ? phase : 0u; row = row0;                   // due == 0: never (a step's 1-based number is compared with it)
    }
    __device__ __forceinline__ void after_step(uint32_t k, const float (&s)[HYDRO_STATE_FIELDS], const float (&f6)[HYDRO_WRENCH_FIELDS])
    {
        if (k + 1u != due) return;
        if (watched) {
            float* p = log + (size_t)row * fields * log_stride + column;
#pragma unroll
            for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) p[(size_t)f * log_stride] = s[f];
            if (fields > (uint32_t)HYDRO_STATE_FIELDS) {
#pragma unroll
                for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) p[(size_t)(HYDRO_STATE_FIELDS + f) * log_stride] = f6[f];
            }
        }
        due += every;
        row += 1u;
    }
};

__device__ __forceinline__ LogRecorder log_recorder(HYDRO_REC_PARAMS)
{
    return LogRecorder{w_mask, w_first, log, log_stride, fields, every, phase, row0, false, 0u, 0u, 0u};
}

template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) step_fused_multi_tiled_kernel(HYDRO_BASE_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, NoRecorder{}, NoApplied{}, NoSea{}, NoBed{}, NoMooring{}, NoExtremes{}, NoTether{});
}

// Same first 16 argument dwords (kernarg preload), the recorder's arguments behind them.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) step_fused_multi_rec_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, log_recorder(HYDRO_REC_ARGS), NoApplied{}, NoSea{}, NoBed{}, NoMooring{}, NoExtremes{}, NoTether{});
}

// --------------------------------------------------------------------------
// The APPLIED WRENCH in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_app): what pushes a body besides
// water and gravity - a thruster, a tether, an RL action.  Six floats per body, a = [Fx Fy Fz | Tx Ty Tz], force at and
// torque about the body origin, in a tiled 6-field record ([tiles][6][64], addressed like the previous-velocity record:
// wave-uniform tile base, field offsets in the load's immediate), held constant IN ITS FRAME for all the steps of a launch:
//   world frame : f6[i] += a[i]                               one fp32 add per component
//   body frame  : f6[0:3] += R a[0:3], f6[3:6] += R a[3:6]    R = the fp32 matrix of the CURRENT step's quaternion, as given
//                                                             (non-unit included), in the form integrate_body builds it -
//                                                             a body-fixed thrust turns with the body inside the launch
// The sum is what the integrator takes (with IMPLICIT it stands where f stood) and what the recorder logs: the wrench that
// produced the state.  The safety clamp has already acted, on the hydrodynamic wrench alone.  `body_frame` is a kernel
// argument, hence wave-uniform: one scalar branch per step.
// The six values are loaded once and carried through the loop (see DESIGN.md for the register counts).
// --------------------------------------------------------------------------
struct AppliedWrench {
    const float* rec; uint32_t stride; int body_frame;
    float a[HYDRO_WRENCH_FIELDS];
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4)
    {
        const float* r = rec + (size_t)tile * stride;
#pragma unroll
        for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) a[f] = ldg<false>(at<float>(r, lane4, f * 256u));
    }
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        if (body_frame) {
            const auto [r00, r01, r02, r10, r11, r12, r20, r21, r22] = rotation_of(s[3], s[4], s[5], s[6]);
#pragma unroll
            for (int h = 0; h < HYDRO_WRENCH_FIELDS; h += 3) {
                f6[h + 0] += r00 * a[h] + r01 * a[h + 1] + r02 * a[h + 2];
                f6[h + 1] += r10 * a[h] + r11 * a[h + 1] + r12 * a[h + 2];
                f6[h + 2] += r20 * a[h] + r21 * a[h + 1] + r22 * a[h + 2];
            }
        } else {
#pragma unroll
            for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) f6[f] += a[f];
        }
    }
};
// The recorder of the applied kernel: LogRecorder, or nothing when there are no watch tables (w_mask == nullptr, a kernel
// argument: wave-uniform) - one kernel serves "applied" and "applied + recorder".
struct OptionalLogRecorder : LogRecorder {
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane)
    {
        if (w_mask) LogRecorder::begin(tile, lane);
        else { watched = false; column = 0u; due = 0u; row = row0; }
    }
};
__device__ __forceinline__ OptionalLogRecorder optional_recorder(HYDRO_REC_PARAMS) { return OptionalLogRecorder{log_recorder(HYDRO_REC_ARGS)}; }

// Same first 16 argument dwords (kernarg preload), the recorder's arguments behind them, then the applied wrench's.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) step_fused_multi_app_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), AppliedWrench{HYDRO_APP_ARGS, {}},
                                                   NoSea{}, NoBed{}, NoMooring{}, NoExtremes{}, NoTether{});
}

// --------------------------------------------------------------------------
// SLOTS floats per lane PARKED IN LDS for the length of a launch, [wave][SLOTS][64] (stride 1 across the lanes: no bank
// conflict): what a policy needs in every step and the loop has no registers for.  A lane reads only what it wrote itself: no
// barrier.  claim(), once per launch, and parked(), in every step, give the address of the lane's slot 0; slot j is
// [j * 64], in the instruction's immediate.  The address is lane4 (live anyway, for the final stores) + a wave-uniform
// scalar, added anew in every step: the empty asm makes the scalar opaque, so that the compiler neither hoists the sum into
// a register of its own nor forwards the parked values through registers.
// --------------------------------------------------------------------------
template <uint32_t SLOTS>
struct LaneSlots {
    uint32_t lane4, wave_off;
    static __device__ __forceinline__ float* slots()
    {
        __shared__ __attribute__((aligned(16))) float lds[kBlock * SLOTS];
        return lds;
    }
    __device__ __forceinline__ float* claim(uint32_t lane4_)
    {
        lane4 = lane4_;
        wave_off = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * (SLOTS * 256u);
        return at<float>(slots(), lane4 + wave_off);
    }
    __device__ __forceinline__ float* parked() const
    {
        uint32_t w_off = wave_off;
        asm volatile("" : "+s"(w_off));
        return at<float>(slots(), lane4 + w_off);
    }
};

// --------------------------------------------------------------------------
// The POSE HOLD in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_ctl): a feedback law evaluated in every
// step from the state the step starts from - between the first and the last step of a launch that state exists nowhere but
// here.  Per body a tiled 17-field control record ([tiles][17][64], addressed like the applied record):
//   p*(3) | q*(4) | kp_lin(3) | kd_lin(3) | kp_ang | kd_ang | f_max | t_max
// The law, in fp32, in this order (include/hydro.h restates it; fma(a, b, c) = a * b + c rounded once):
//   e_i  = p*_i - p_i                          F_i = fma(kp_lin_i, e_i, -(kd_lin_i * v_i))
//   n2   = fma(F_z, F_z, fma(F_y, F_y, F_x * F_x));          if (n2 > f_max * f_max)  F_i *= f_max * rsqrt_nr(n2)
//   q_e  = q* (x) conj(q):   w = fma(tw, qw, fma(tx, qx, fma(ty, qy, tz * qz)))                    (t = q*)
//                            x = fma(qw, tx, fma(-tw, qx, fma(qy, tz, -(qz * ty))))   y, z: the cyclic successors
//   h    = w < 0 ? -2 : 2                      T_i = fma(kp_ang, h * q_e_i, -(kd_ang * omega_i))
//   n2, clamp to t_max as for F;               f6[0:3] += F, f6[3:6] += T
// after the applied wrench, if there is one.  The sum is what the integrator takes and what the recorder logs.
// WHERE THE 17 VALUES LIVE: the applied kernels stand at 156-168 VGPRs, at the limit of 3 waves per SIMD, so the record is
// not carried through the loop.  Each lane parks its record - and the six applied values, which this kernel does not carry
// either - in LDS once per launch and reads them back in every step: 23 slots per lane, [wave][23][64] floats (23 KB per
// block; LaneSlots, above).
// The kernel asks for 3 waves per SIMD (amdgpu_waves_per_eu(3)): left to itself the scheduler spends 170 VGPRs on the
// energy-sampling instantiations - two more than three waves allow - where 160 do, without scratch (138-160 over the 32).
// --------------------------------------------------------------------------
constexpr uint32_t kCtlSlots = HYDRO_CTL_FIELDS + HYDRO_WRENCH_FIELDS;
struct PoseHold : LaneSlots<kCtlSlots> {
    const float* ctl; uint32_t ctl_stride; const float* applied; uint32_t applied_stride; int body_frame;
    // the six applied values: slots 17 .. 22
    __device__ __forceinline__ void park_applied(float* mine, uint32_t tile) const
    {
        const float* a = applied + (size_t)tile * applied_stride;
#pragma unroll
        for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) mine[(HYDRO_CTL_FIELDS + f) * 64] = ldg<false>(at<float>(a, lane4, f * 256u));
    }
    __device__ __forceinline__ void add_parked_applied(const float* mine, const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        // (an AppliedWrench as the carrier of the six values: handing them to a free function as a bare array computes the same
        // and moves registers in the 64 pose-hold and sea kernels)
        AppliedWrench a{nullptr, 0u, body_frame, {}};
#pragma unroll
        for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) a.a[f] = mine[(HYDRO_CTL_FIELDS + f) * 64];
        a.add(s, f6);
    }
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        float* mine = claim(lane4_);
        const float* r = ctl + (size_t)tile * ctl_stride;
#pragma unroll
        for (int f = 0; f < HYDRO_CTL_FIELDS; ++f) mine[f * 64] = ldg<false>(at<float>(r, lane4, f * 256u));
        if (applied) park_applied(mine, tile);               // (a kernel argument: wave-uniform)
        else {
#pragma unroll
            for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) mine[(HYDRO_CTL_FIELDS + f) * 64] = 0.0f;
        }
    }
    static __device__ __forceinline__ void clamp_norm(float (&v)[3], float top)
    {
        const float n2 = __builtin_fmaf(v[2], v[2], __builtin_fmaf(v[1], v[1], v[0] * v[0]));
        if (n2 > top * top) {
            const float k = top * rsqrt_nr(n2);
            v[0] *= k; v[1] *= k; v[2] *= k;
        }
    }
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        const float* mine = parked();
        add_parked_applied(mine, s, f6);
        {
            float F[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) F[i] = __builtin_fmaf(mine[(7 + i) * 64], mine[i * 64] - s[i], -(mine[(10 + i) * 64] * s[7 + i]));
            clamp_norm(F, mine[15 * 64]);
#pragma unroll
            for (int i = 0; i < 3; ++i) f6[i] += F[i];
        }
        const float tx = mine[3 * 64], ty = mine[4 * 64], tz = mine[5 * 64], tw = mine[6 * 64], qx = s[3], qy = s[4], qz = s[5], qw = s[6];
        const float ew = __builtin_fmaf(tw, qw, __builtin_fmaf(tx, qx, __builtin_fmaf(ty, qy, tz * qz)));
        const float ex = __builtin_fmaf(qw, tx, __builtin_fmaf(-tw, qx, __builtin_fmaf(qy, tz, -(qz * ty))));
        const float ey = __builtin_fmaf(qw, ty, __builtin_fmaf(-tw, qy, __builtin_fmaf(qz, tx, -(qx * tz))));
        const float ez = __builtin_fmaf(qw, tz, __builtin_fmaf(-tw, qz, __builtin_fmaf(qx, ty, -(qy * tx))));
        const float h = ew < 0.0f ? -2.0f : 2.0f, kp = mine[13 * 64], kd = mine[14 * 64];
        float T[3] = {__builtin_fmaf(kp, h * ex, -(kd * s[10])), __builtin_fmaf(kp, h * ey, -(kd * s[11])), __builtin_fmaf(kp, h * ez, -(kd * s[12]))};
        clamp_norm(T, mine[16 * 64]);
#pragma unroll
        for (int i = 0; i < 3; ++i) f6[3 + i] += T[i];
    }
};

__device__ __forceinline__ PoseHold pose_hold(HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS)
{
    return PoseHold{{0u, 0u}, control, control_stride, applied, applied_stride, body_frame};
}

// The applied kernel's arguments, then the control record's.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_ctl_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   NoSea{}, NoBed{}, NoMooring{}, NoExtremes{}, NoTether{});
}

// --------------------------------------------------------------------------
// The SEA STATE in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_sea): a steady uniform current and up to
// HYDRO_SEA_WAVES_MAX regular deep-water wave components, scene-wide like rho and g (hydro_set_sea).  The wrench is
// translation-invariant in x, y and sees the water only through the depth of the body centre and the body's velocity, so moving
// water is body_wrench of a RELATIVE state: p_z below the local surface, v and the previous v against the local water.  The
// wave phase advances with every step and the states between the ends of a launch exist in registers only: the view is
// formed here, per step.  include/hydro.h states the order of operations; sea_water below is its ONLY implementation (the
// step kernel and hydro_sea_sample's kernel both call it).
//   table : the engine's device copy of the sea, read through the CONSTANT address space: wave-uniform addresses, hence
//           scalar loads (s_load) in every step - the components take no vector registers between steps
//   time  : t = (step0 + k) * dt in fp64, tau_j = phi_j - omega_j t reduced by a two-term 2 pi in fp64 (error about
//           1e-16 |omega_j t|: 5e-12 rad after 10^6 steps at 60 Hz), THEN rounded to fp32
//   trig  : the hardware seeds v_sin_f32 / v_cos_f32 (argument in revolutions) behind an explicit reduction
//           r = th / 2 pi - rint(th / 2 pi), exact but for the one product; v_exp_f32 for the depth decay
// WHERE THE TRUE STATE LIVES while the wrench runs: the applied kernels stand at the limit of 3 waves per SIMD, so the seven
// true values (p_z, v, pv[0:3]) are parked in LDS around body_wrench, [wave][7][64] floats (7 KB per block), and the relative
// ones take their registers - no live range is added to the wrench (LaneSlots, above).
// --------------------------------------------------------------------------
struct SeaWave {
    double omega, phi;                                   // rad / s, rad
    float a, kx, ky, kl2, cx, cy, aw, pad;               // amplitude, wave vector, kappa log2(e), a omega kx / kappa, a omega ky / kappa, a omega
};
struct SeaTable {
    float u[3]; uint32_t waves;
    SeaWave w[HYDRO_SEA_WAVES_MAX];
};
typedef const __attribute__((address_space(4))) SeaTable* SeaTablePtr;
__device__ __forceinline__ SeaTablePtr sea_table_ptr(const void* p) { return (SeaTablePtr)p; }

// eta and u of the water at (px, py) for a body whose centre is at pz, at the start of step `step` (include/hydro.h, "sea").
__device__ __forceinline__ void sea_water(SeaTablePtr tab, uint32_t waves, int64_t step, double dt, float px, float py, float pz,
                                          float& eta, float (&u)[3])
{
    constexpr double kInv2Pi = 0.15915494309189535, kTwoPiHi = 6.283185307179586, kTwoPiLo = 2.4492935982947064e-16;
    const double t = (double)step * dt;
    float cs[HYDRO_SEA_WAVES_MAX], sn[HYDRO_SEA_WAVES_MAX];
    eta = 0.0f;
#pragma unroll
    for (int j = 0; j < HYDRO_SEA_WAVES_MAX; ++j) {
        if ((uint32_t)j < waves) {                           // (wave-uniform)
            const double x = __builtin_fma(-tab->w[j].omega, t, tab->w[j].phi);
            const double m = __builtin_rint(x * kInv2Pi);
            const float tau = (float)__builtin_fma(-m, kTwoPiLo, __builtin_fma(-m, kTwoPiHi, x));
            const float th = __builtin_fmaf(tab->w[j].kx, px, __builtin_fmaf(tab->w[j].ky, py, tau));
            const float rev = th * 0.15915494309189535f;
            const float r = rev - __builtin_rintf(rev);
            cs[j] = __builtin_amdgcn_cosf(r);
            sn[j] = __builtin_amdgcn_sinf(r);
            eta = __builtin_fmaf(tab->w[j].a, cs[j], eta);
        }
    }
    const float zc = __builtin_fminf(pz - eta, 0.0f);
    u[0] = tab->u[0]; u[1] = tab->u[1]; u[2] = tab->u[2];
#pragma unroll
    for (int j = 0; j < HYDRO_SEA_WAVES_MAX; ++j) {
        if ((uint32_t)j < waves) {
            const float e = __builtin_amdgcn_exp2f(tab->w[j].kl2 * zc);
            const float ec = e * cs[j], es = e * sn[j];
            u[0] = __builtin_fmaf(tab->w[j].cx, ec, u[0]);
            u[1] = __builtin_fmaf(tab->w[j].cy, ec, u[1]);
            u[2] = __builtin_fmaf(tab->w[j].aw, es, u[2]);
        }
    }
}

constexpr uint32_t kSeaSlots = 7;
struct SeaView : LaneSlots<kSeaSlots> {
    SeaTablePtr tab; uint32_t waves; int64_t step0; double dt;
    __device__ __forceinline__ void begin(uint32_t lane4_) { claim(lane4_); }
    __device__ __forceinline__ void view(uint32_t k, float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS]) const
    {
        float eta, u[3];
        sea_water(tab, waves, step0 + (int64_t)k, dt, s[0], s[1], s[2], eta, u);
        float* m = parked();
        m[0] = s[2];
        s[2] = s[2] - eta;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            m[(1 + i) * 64] = s[7 + i];
            m[(4 + i) * 64] = pv[i];
            s[7 + i] = s[7 + i] - u[i];
            pv[i] = pv[i] - u[i];
        }
    }
    __device__ __forceinline__ void restore(float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS]) const
    {
        const float* m = parked();
        s[2] = m[0];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            s[7 + i] = m[(1 + i) * 64];
            pv[i] = m[(4 + i) * 64];
        }
    }
};

// The pose hold of the sea kernel: `control` and `applied` are each optional (kernel arguments: wave-uniform branches), and
// what is added is what the kernel the host would pick WITHOUT a sea adds - PoseHold with a control record (zeros for a
// missing applied wrench, as there), the applied wrench alone without one, nothing without either.
struct OptionalPoseHold : PoseHold {
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        if (ctl) { PoseHold::begin(tile, lane4_); return; }
        float* mine = claim(lane4_);
        if (applied) park_applied(mine, tile);
    }
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        if (ctl) { PoseHold::add(s, f6); return; }
        if (applied) add_parked_applied(parked(), s, f6);
    }
};
__device__ __forceinline__ OptionalPoseHold optional_pose_hold(HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS) { return OptionalPoseHold{pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS)}; }
__device__ __forceinline__ SeaView sea_view(HYDRO_SEA_PARAMS) { return SeaView{{0u, 0u}, sea_table_ptr(sea_table), sea_waves, step0, sea_dt}; }

// The pose-hold kernel's arguments, then the sea's.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_sea_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                 HYDRO_SEA_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   sea_view(HYDRO_SEA_ARGS), NoBed{}, NoMooring{}, NoExtremes{}, NoTether{});
}

// hydro_sea_sample: [eta, u_x, u_y, u_z] per body, the values a step that starts from `st` at step index `step` uses.
__global__ void __launch_bounds__(kBlock) sea_sample_kernel(const float* st, uint32_t st_stride, float* out, uint32_t out_stride, uint32_t n,
                                                            const void* sea_table, uint32_t sea_waves, int64_t step, double sea_dt)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const float* r = st + (size_t)tile * st_stride;
    float eta, u[3];
    sea_water(sea_table_ptr(sea_table), sea_waves, step, sea_dt, *at<float>(r, lane4, 0u), *at<float>(r, lane4, 256u), *at<float>(r, lane4, 512u), eta, u);
    const float o[HYDRO_SEA_FIELDS] = {eta, u[0], u[1], u[2]};
    store_record<HYDRO_SEA_FIELDS, false>(out + (size_t)tile * out_stride, lane4, o);
}

// --------------------------------------------------------------------------
// The sea in the OPEN-LOOP steps (hydro_step_wrench_tiled_sea, hydro_step_wrench_aos_sea): the wrench-only kernels with the
// view formed between their loads and body_wrench.  New kernels beside wrench_tiled_kernel and wrench_aos_direct_kernel, which
// stay as they are (their instruction budget is the headline's); the host launches these only while a sea is set.
//   time  : the caller's, in seconds, handed over as (step, sea_dt) with (double)step * sea_dt == time exactly - step = 1,
//           sea_dt = time, or step = 0 at time 0 - so that sea_water stays the only implementation of the view.
//   prev  : single-step kernels, nothing is parked: the TRUE velocity goes to the engine's record before the view is formed
//           (its stores are issued early and no true value stays live across body_wrench); a caller-owned record is only read.
// --------------------------------------------------------------------------
__device__ __forceinline__ void sea_relative(SeaTablePtr tab, uint32_t waves, int64_t step, double sea_dt,
                                             float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS])
{
    float eta, u[3];
    sea_water(tab, waves, step, sea_dt, s[0], s[1], s[2], eta, u);
    s[2] = s[2] - eta;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s[7 + i] = s[7 + i] - u[i];
        pv[i] = pv[i] - u[i];
    }
}

// wrench_tiled_kernel<256, HALF, ENGINE_PREV, NT, no KE, WARP>'s arguments (the same 16 preloaded dwords), then the sea's.
template <bool HALF, bool ENGINE_PREV, bool NT, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_TILED_OCC_ATTR wrench_tiled_sea_kernel(const float* k_st, const float* k_pv, const float* k_prm, float* k_out, float* k_pv_out,
                                                             uint32_t st_stride, uint32_t pv_stride, uint32_t out_stride, uint32_t pvo_stride,
                                                             uint32_t n, int warp, double rho, double g, double inv_dt,
                                                             const void* sea_table, uint32_t sea_waves, int64_t step, double sea_dt)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u;
    const uint32_t first = tile * 64u;
    const uint32_t left = n - __builtin_amdgcn_readfirstlane(n < first ? n : first);       // (scalar, see wrench_tiled_kernel)
    if (lane >= left) return;
    const uint32_t lane4 = lane * 4u;
    float s[HYDRO_STATE_FIELDS], pv[HYDRO_PREV_FIELDS], d[3], c[7], mass, f6[HYDRO_WRENCH_FIELDS];
    load_tile_records<HALF, NT>(k_st + (size_t)tile * st_stride, k_pv + (size_t)tile * pv_stride, k_prm, tile, lane4, s, pv, d, c, mass);
    if constexpr (ENGINE_PREV) store_record<HYDRO_PREV_FIELDS, NT>(k_pv_out + (size_t)tile * pvo_stride, lane4, s + 7);
    sea_relative(sea_table_ptr(sea_table), sea_waves, step, sea_dt, s, pv);
    wrench_fields(body_wrench(s, pv, d, c, mass, rho, g, inv_dt, WARP), f6);
    store_record<HYDRO_WRENCH_FIELDS, NT>(k_out + (size_t)tile * out_stride, lane4, f6);
}

// wrench_aos_direct_kernel's arguments and frame - the same row accesses, temporal row loads - then the sea's.
template <bool HALF, bool NT, bool WARP>
__global__ void __launch_bounds__(kBlock) wrench_aos_sea_kernel(const float* k_pos, const float* k_quat, const float* k_vel, float* k_force, float* k_torque,
                                                               float* k_pv, const float* k_prm, int quat_xyzw, uint32_t n,      // 16 dwords: preloaded
                                                               int warp, double rho, double g, double inv_dt,
                                                               const void* sea_table, uint32_t sea_waves, int64_t step, double sea_dt)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const size_t first = (size_t)tile * 64u;
    const float* t_pos = k_pos + first * 3; const float* t_quat = k_quat + first * 4; const float* t_vel = k_vel + first * 6;
    float s[HYDRO_STATE_FIELDS], pv[HYDRO_PREV_FIELDS], d[3], c[7], mass;
    constexpr bool RNT = false;                              // (the simulator's rows: temporal, see wrench_aos_direct_kernel)
    const f3_a4 p = ld_f3_a4<RNT>(t_pos, lane * 12u);
    const f4_a16 q = ld_f4_a16<RNT>(t_quat, lane * 16u);
    const f4_a8 v0 = ld_f4_a8<RNT>(t_vel, lane * 24u);
    const f2_a8 v1 = ld_f2_a8<RNT>(t_vel, lane * 24u + 16u);
    s[0] = p.x; s[1] = p.y; s[2] = p.z;
    if (quat_xyzw) { s[3] = q.x; s[4] = q.y; s[5] = q.z; s[6] = q.w; }
    else           { s[3] = q.y; s[4] = q.z; s[5] = q.w; s[6] = q.x; }
    s[7] = v0.x; s[8] = v0.y; s[9] = v0.z; s[10] = v0.w; s[11] = v1.x; s[12] = v1.y;
    float* t_pv = k_pv + (size_t)tile * (HYDRO_PREV_FIELDS * HYDRO_TILE);
#pragma unroll
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) pv[f] = ldg<NT>(at<float>(t_pv, lane4, f * 256u));
    load_param_record<HALF, NT>(k_prm, tile, lane4, d, c, mass);
#pragma unroll
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) stg_aos<NT>(at<float>(t_pv, lane4, f * 256u), s[7 + f]);     // the TRUE velocity
    sea_relative(sea_table_ptr(sea_table), sea_waves, step, sea_dt, s, pv);
    const hydro::Wrench w = body_wrench(s, pv, d, c, mass, rho, g, inv_dt, WARP);
    f3_a4 fo, to;
    fo.x = w.fx; fo.y = w.fy; fo.z = w.fz; to.x = w.tx; to.y = w.ty; to.z = w.tz;
    st_f3_a4<NT>(k_force + first * 3, lane * 12u, fo);
    st_f3_a4<NT>(k_torque + first * 3, lane * 12u, to);
}

// --------------------------------------------------------------------------
// The SEABED in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_bed): the horizontal plane z = z_b under the
// water, scene-wide like rho, g and the sea (hydro_set_seabed).  A body touches it through the eight corners of the box the
// buoyancy already uses: per corner below the plane a mass-normalised spring and damper along z (no adhesion) and a Coulomb
// friction whose direction is regularised by a slip speed and whose tangential damping is capped.  include/hydro.h states
// the model and the order of operations ("Seabed"); seabed_wrench below is its ONLY implementation (the step kernel and
// hydro_seabed_wrench's kernel both call it).  The bed sees the TRUE state - never the one relative to the water - and adds
// its wrench behind the applied wrench and the pose hold, in front of the integrator: one fp32 add per component.
//   constants   : six floats, rounded once on the host, kernel arguments (SGPRs) - no table
//   broad phase : the lowest corner stands at p_z - ((|A_z| + |B_z|) + |C_z|), A_z = R_20 dx/2 ... - and that is, bit for
//                 bit, the t_i of the corner whose signs oppose those of A_z, B_z, C_z: fp32 rounding is monotone and
//                 symmetric, so no other corner's t_i lies below it.  delta_max = z_b - that value is therefore EXACTLY the
//                 largest delta_i (margin 0 is conservative), and a lane whose delta_max is not > 0 has no contributing
//                 corner.  If that holds for every lane of the wavefront (ballot == 0) the wave branches round the contact:
//                 a scene far from the bed pays the rotation's third row, three products, three adds, a compare and the branch
//   the skip    : a lane without a contributing corner leaves f6 untouched (it does not add +0: the sign of a zero
//                 survives), whether its wave took the branch or not - skipped and evaluated give the same bits
// It runs behind the fp64 wrench, where that wrench's registers are free again; nothing is parked for it.
// --------------------------------------------------------------------------
struct Seabed { float z, stiffness, damping, friction, slip_speed, friction_rate; };

// W (force at, torque about the body origin, world frame) of the bed on a body in state s with box d and mass m.  Returns
// whether any corner contributed; W is meaningful (and complete) only then.
__device__ __forceinline__ bool seabed_wrench(const Seabed& b, const float (&s)[HYDRO_STATE_FIELDS], const float (&d)[3], float m,
                                              float (&W)[HYDRO_WRENCH_FIELDS])
{
    const auto [r00, r01, r02, r10, r11, r12, r20, r21, r22] = rotation_of(s[3], s[4], s[5], s[6]);
    // (0.5 * (R d), not R (0.5 d) - the same value, and nothing in it that is constant over the steps of a launch: the compiler
    // would carry such a value through the loop in a register of its own, and the loop has none to spare)
    const float pz0 = r20 * d[0], pz1 = r21 * d[1], pz2 = r22 * d[2];
    const float az = 0.5f * pz0, bz = 0.5f * pz1, cz = 0.5f * pz2;
    const float reach = (__builtin_fabsf(az) + __builtin_fabsf(bz)) + __builtin_fabsf(cz);
    const float lowest = s[2] - reach;
    const bool can_touch = b.z - lowest > 0.0f;
    if (__builtin_amdgcn_ballot_w64(can_touch) == 0) return false;        // (scalar branch: nobody in this wave is near the bed)
    const float px0 = r00 * d[0], px1 = r01 * d[1], px2 = r02 * d[2];
    const float py0 = r10 * d[0], py1 = r11 * d[1], py2 = r12 * d[2];
    const float ax = 0.5f * px0, bx = 0.5f * px1, cx = 0.5f * px2;
    const float ay = 0.5f * py0, by = 0.5f * py1, cy = 0.5f * py2;
    bool any = false;
#pragma unroll
    for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) W[f] = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float sx = (i & 1) ? 1.0f : -1.0f, sy = (i & 2) ? 1.0f : -1.0f, sz = (i & 4) ? 1.0f : -1.0f;
        const float rx = __builtin_fmaf(sz, cx, __builtin_fmaf(sy, bx, sx * ax));
        const float ry = __builtin_fmaf(sz, cy, __builtin_fmaf(sy, by, sx * ay));
        const float rz = __builtin_fmaf(sz, cz, __builtin_fmaf(sy, bz, sx * az));
        const float t = s[2] + rz;
        const float delta = b.z - t;
        if (delta > 0.0f) {
            any = true;
            const float ux = __builtin_fmaf(s[11], rz, __builtin_fmaf(-s[12], ry, s[7]));
            const float uy = __builtin_fmaf(s[12], rx, __builtin_fmaf(-s[10], rz, s[8]));
            const float uz = __builtin_fmaf(s[10], ry, __builtin_fmaf(-s[11], rx, s[9]));
            const float bu = b.damping * uz;
            const float a = __builtin_fmaf(b.stiffness, delta, -bu);
            const float ap = __builtin_fmaxf(0.0f, a);
            const float N = m * ap;
            const float mua = b.friction * ap;
            const float ux2 = ux * ux;
            const float ut2 = __builtin_fmaf(b.slip_speed, b.slip_speed, __builtin_fmaf(uy, uy, ux2));
            const float q = mua * rsqrt_nr(ut2);
            const float c = m * __builtin_fminf(q, b.friction_rate);
            const float tx = c * ux, ty = c * uy;                             // F = (-tx, -ty, N)
            W[0] = W[0] - tx;
            W[1] = W[1] - ty;
            W[2] = W[2] + N;
            W[3] = __builtin_fmaf(ry, N, __builtin_fmaf(rz, ty, W[3]));
            W[4] = __builtin_fmaf(-rz, tx, __builtin_fmaf(-rx, N, W[4]));
            W[5] = __builtin_fmaf(ry, tx, __builtin_fmaf(-rx, ty, W[5]));
        }
    }
    return any;
}

struct SeabedContact {
    Seabed b;
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], const float (&d)[3], float mass, float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        float W[HYDRO_WRENCH_FIELDS];
        if (seabed_wrench(b, s, d, mass, W)) {
#pragma unroll
            for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) f6[f] += W[f];
        }
    }
};

// The sea of the bed kernel: optional (a null table - a kernel argument: wave-uniform); an absent sea forms no view and
// parks nothing, so the wrench takes the true state as in the kernels without a sea.
struct OptionalSeaView : SeaView {
    __device__ __forceinline__ void view(uint32_t k, float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS]) const
    {
        if (tab) SeaView::view(k, s, pv);
    }
    __device__ __forceinline__ void restore(float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS]) const
    {
        if (tab) SeaView::restore(s, pv);
    }
};
__device__ __forceinline__ OptionalSeaView optional_sea_view(HYDRO_SEA_PARAMS) { return OptionalSeaView{sea_view(HYDRO_SEA_ARGS)}; }
__device__ __forceinline__ SeabedContact seabed_contact(HYDRO_BED_PARAMS) { return SeabedContact{{HYDRO_BED_ARGS}}; }

// The sea kernel's arguments, then the bed's six constants.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_bed_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                 HYDRO_SEA_PARAMS, HYDRO_BED_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   optional_sea_view(HYDRO_SEA_ARGS), seabed_contact(HYDRO_BED_ARGS), NoMooring{}, NoExtremes{}, NoTether{});
}

// hydro_seabed_wrench: the bed's W per body for the tiled state `st` (zeros for a body no corner of which is below the plane).
__global__ void __launch_bounds__(kBlock) seabed_wrench_kernel(const float* st, uint32_t st_stride, const float* prm, uint32_t prm_tile_floats, uint32_t mass_field,
                                                               float* out, uint32_t out_stride, uint32_t n, Seabed bed)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const float* r = st + (size_t)tile * st_stride;
    const float* q = prm + (size_t)tile * prm_tile_floats + lane;
    float s[HYDRO_STATE_FIELDS], W[HYDRO_WRENCH_FIELDS];
#pragma unroll
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) s[f] = *at<float>(r, lane4, f * 256u);
    const float d[3] = {q[0], q[64], q[128]};
    if (!seabed_wrench(bed, s, d, q[mass_field * 64u], W)) {
#pragma unroll
        for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) W[f] = 0.0f;
    }
    store_record<HYDRO_WRENCH_FIELDS, false>(out + (size_t)tile * out_stride, lane4, W);
}

// --------------------------------------------------------------------------
// MOORING LINES in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_moor): per body ONE tension-only line
// from an anchor fixed in the world to a fairlead fixed in the body - a spring and a damper along the line that never push.
// Per body a tiled 9-field record ([tiles][9][64], addressed like the control record):
//   a(3) | b(3) | L0 | k | c
// include/hydro.h states the model and the order of operations ("Mooring"); mooring_wrench below is its ONLY implementation
// (the step kernel and hydro_mooring_wrench's kernel both call it).  The line sees the TRUE state - never the one relative
// to the water - and adds its wrench behind the bed, in front of the integrator: one fp32 add per component.
//   the record  : the caller's device buffer, read at every launch.  The bed kernels stand at 161-167 VGPRs against the 168
//                 of three waves per SIMD, so the nine values are not carried through the loop: each lane parks them in LDS
//                 once per launch, [wave][9][64] floats (9 KB per block; LaneSlots, above), and reads them back in every step
//   the skip    : a lane has a line if k > 0 or c > 0.  If no lane of the wavefront has one (ballot == 0) the wave branches
//                 round the evaluation: an unmoored scene pays two LDS reads, two compares and the branch
//   no +0       : a lane whose line adds nothing (no line, slack, or a tension that is not > 0) leaves f6 untouched, whether
//                 its wave took the branch or not - skipped and evaluated give the same bits
// It runs behind the fp64 wrench and the bed, where their registers are free again.
// --------------------------------------------------------------------------
// W (force at, torque about the body origin, world frame) of the line whose record is m[j * 64], j = 0 .. 8, on a body in
// state s.  Returns whether the line pulls; W is meaningful (and complete) only then, and so is `tension`, the T W was
// formed from (the extremes record keeps its maximum; a wave that skips leaves it untouched).
__device__ __forceinline__ bool mooring_wrench(const float* m, const float (&s)[HYDRO_STATE_FIELDS], float (&W)[HYDRO_WRENCH_FIELDS], float& tension)
{
    const float k = m[7 * 64], c = m[8 * 64];
    const bool has_line = k > 0.0f || c > 0.0f;
    if (__builtin_amdgcn_ballot_w64(has_line) == 0) return false;         // (scalar branch: nobody in this wave is moored)
    const auto [r00, r01, r02, r10, r11, r12, r20, r21, r22] = rotation_of(s[3], s[4], s[5], s[6]);
    const float bx = m[3 * 64], by = m[4 * 64], bz = m[5 * 64];
    const float rx = __builtin_fmaf(r02, bz, __builtin_fmaf(r01, by, r00 * bx));
    const float ry = __builtin_fmaf(r12, bz, __builtin_fmaf(r11, by, r10 * bx));
    const float rz = __builtin_fmaf(r22, bz, __builtin_fmaf(r21, by, r20 * bx));
    const float ex = (m[0 * 64] - s[0]) - rx, ey = (m[1 * 64] - s[1]) - ry, ez = (m[2 * 64] - s[2]) - rz;
    const float l2 = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    const float inv = rsqrt_nr(l2);
    const float l = l2 * inv;
    const float x = l - m[6 * 64];
    const float ux = __builtin_fmaf(s[11], rz, __builtin_fmaf(-s[12], ry, s[7]));
    const float uy = __builtin_fmaf(s[12], rx, __builtin_fmaf(-s[10], rz, s[8]));
    const float uz = __builtin_fmaf(s[10], ry, __builtin_fmaf(-s[11], rx, s[9]));
    const float un = __builtin_fmaf(uz, ez, __builtin_fmaf(uy, ey, ux * ex)) * inv;
    const float cu = c * un;
    const float T = __builtin_fmaxf(0.0f, __builtin_fmaf(k, x, -cu));
    const float ti = T * inv;
    tension = T;
    W[0] = ti * ex; W[1] = ti * ey; W[2] = ti * ez;
    W[3] = __builtin_fmaf(ry, W[2], -(rz * W[1]));
    W[4] = __builtin_fmaf(rz, W[0], -(rx * W[2]));
    W[5] = __builtin_fmaf(rx, W[1], -(ry * W[0]));
    return has_line && x > 0.0f && T > 0.0f;                              // (l2 = 0: x is NaN, not taut)
}
__device__ __forceinline__ bool mooring_wrench(const float* m, const float (&s)[HYDRO_STATE_FIELDS], float (&W)[HYDRO_WRENCH_FIELDS])
{
    float tension;
    return mooring_wrench(m, s, W, tension);
}

constexpr uint32_t kMoorSlots = HYDRO_MOOR_FIELDS;
struct MooringLine : LaneSlots<kMoorSlots> {
    const float* rec; uint32_t stride;
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        float* mine = claim(lane4_);
        const float* r = rec + (size_t)tile * stride;
#pragma unroll
        for (int f = 0; f < HYDRO_MOOR_FIELDS; ++f) mine[f * 64] = ldg<false>(at<float>(r, lane4, f * 256u));
    }
    // Behind the loop of a kernel that samples the kinetic energy: the box as the energy sees it is made opaque.  The energy
    // takes (double)d, which the fp64 wrench forms in front of the loop too; left to itself the compiler keeps those doubles
    // alive across the loop for the energy's sake - four VGPRs the loop does not have (it spilled them to scratch).  Behind
    // the empty asm the conversions are made anew from the floats, which are live anyway.  Same values, same bits.
    __device__ __forceinline__ void end(float (&d)[3]) const
    {
        asm volatile("" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]));
    }
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        float W[HYDRO_WRENCH_FIELDS];
        if (mooring_wrench(parked(), s, W)) {
#pragma unroll
            for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) f6[f] += W[f];
        }
    }
    __device__ __forceinline__ float tension() const { return 0.0f; }        // (nobody asks: the mooring kernels track no extremes)
};

// The bed of the mooring kernel: optional (`present` - a kernel argument: wave-uniform); an absent bed runs no broad phase
// and adds nothing, the bits of the kernels without one.
struct OptionalSeabedContact : SeabedContact {
    int present;
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], const float (&d)[3], float mass, float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        if (present) SeabedContact::add(s, d, mass, f6);
    }
};
__device__ __forceinline__ OptionalSeabedContact optional_seabed_contact(HYDRO_OPT_BED_PARAMS) { return OptionalSeabedContact{seabed_contact(HYDRO_BED_ARGS), bed_present}; }
__device__ __forceinline__ MooringLine mooring_line(HYDRO_MOOR_PARAMS) { return MooringLine{{0u, 0u}, mooring, mooring_stride}; }

// The bed kernel's arguments, then the bed's presence, then the mooring record's.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_moor_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                  HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_MOOR_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   optional_sea_view(HYDRO_SEA_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS), mooring_line(HYDRO_MOOR_ARGS),
                                                   NoExtremes{}, NoTether{});
}

// hydro_mooring_wrench: the line's W per body for the tiled state `st` (+0 in all six fields for a body whose line adds nothing).
__global__ void __launch_bounds__(kBlock) mooring_wrench_kernel(const float* st, uint32_t st_stride, const float* moor, uint32_t moor_stride,
                                                                float* out, uint32_t out_stride, uint32_t n)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const float* r = st + (size_t)tile * st_stride;
    float s[HYDRO_STATE_FIELDS], W[HYDRO_WRENCH_FIELDS];
#pragma unroll
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) s[f] = *at<float>(r, lane4, f * 256u);
    if (!mooring_wrench(moor + (size_t)tile * moor_stride + lane, s, W)) {
#pragma unroll
        for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) W[f] = 0.0f;
    }
    store_record<HYDRO_WRENCH_FIELDS, false>(out + (size_t)tile * out_stride, lane4, W);
}

// --------------------------------------------------------------------------
// EXTREMES in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_ext): what a design-load study asks of a long
// resident run - how far, how deep, how fast, how hard did the line pull - without a trajectory.  Per body a tiled 8-field
// record ([tiles][8][64], addressed like the mooring record):
//   x_min x_max | y_min y_max | z_min z_max | speed2_max | tension_max
// include/hydro.h states the sample and the update ("Extremes").  Unlike every other record it is READ at the start of a
// launch and WRITTEN at its end: the extremes accumulate across launches until hydro_extremes_reset.
//   the sample  : after every step, the state the step produced (a recorder row's values) and the tension T that
//                 mooring_wrench formed in that step - handed over by TrackedMooringLine, +0 where the line adds nothing
//   the update  : extreme_min / extreme_max, an explicit compare-and-select (v_cmp + v_cndmask), never fminf / fmaxf: a NaN
//                 sample never enters, a NaN accumulator stays, an equal value (+-0 included) leaves the accumulator's bits
//   the record  : the mooring kernels stand at 161-165 VGPRs of 168, so the eight accumulators are not carried through the
//                 loop: each lane parks them in LDS, [wave][8][64] floats (8 KB per block; LaneSlots), and reads, updates
//                 and writes them behind the integrator, where the fp64 wrench's registers are free
// Nothing the policy computes feeds back: state, prev_out, energy and log are the mooring kernel's bits.
// --------------------------------------------------------------------------
__device__ __forceinline__ float extreme_min(float m, float x) { return (x < m) ? x : m; }
__device__ __forceinline__ float extreme_max(float M, float x) { return (x > M) ? x : M; }

// The line that remembers the tension of its last add: T if the line pulled, +0 if it added nothing.
struct TrackedMooringLine : MooringLine {
    mutable float last;
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        float W[HYDRO_WRENCH_FIELDS], T = 0.0f;
        const bool pulls = mooring_wrench(parked(), s, W, T);
        if (pulls) {
#pragma unroll
            for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) f6[f] += W[f];
        }
        last = pulls ? T : 0.0f;
    }
    __device__ __forceinline__ float tension() const { return last; }
};
// The lines of the extremes kernel: optional (`rec` - a kernel argument: wave-uniform); an absent record parks nothing,
// evaluates nothing and reports a tension of +0.
struct OptionalMooringLine : TrackedMooringLine {
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        if (rec) MooringLine::begin(tile, lane4_);
    }
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        if (rec) TrackedMooringLine::add(s, f6);
        else last = 0.0f;
    }
};

constexpr uint32_t kExtSlots = HYDRO_EXT_FIELDS;
struct ExtremesTrack : LaneSlots<kExtSlots> {
    float* rec; uint32_t stride;
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        float* mine = claim(lane4_);
        const float* r = rec + (size_t)tile * stride;
#pragma unroll
        for (int f = 0; f < HYDRO_EXT_FIELDS; ++f) mine[f * 64] = ldg<false>(at<float>(r, lane4, f * 256u));
    }
    __device__ __forceinline__ void after_step(const float (&s)[HYDRO_STATE_FIELDS], float T) const
    {
        float* e = parked();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            e[(2 * a) * 64] = extreme_min(e[(2 * a) * 64], s[a]);
            e[(2 * a + 1) * 64] = extreme_max(e[(2 * a + 1) * 64], s[a]);
        }
        const float speed2 = __builtin_fmaf(s[9], s[9], __builtin_fmaf(s[8], s[8], s[7] * s[7]));
        e[6 * 64] = extreme_max(e[6 * 64], speed2);
        e[7 * 64] = extreme_max(e[7 * 64], T);
    }
    // Only live lanes come here (fused_multi_body): the padding lanes of the last tile are never written.
    __device__ __forceinline__ void end(uint32_t tile, uint32_t lane4_) const
    {
        const float* e = parked();
        float v[HYDRO_EXT_FIELDS];
#pragma unroll
        for (int f = 0; f < HYDRO_EXT_FIELDS; ++f) v[f] = e[f * 64];
        store_record<HYDRO_EXT_FIELDS, false>(rec + (size_t)tile * stride, lane4_, v);
    }
};

__device__ __forceinline__ OptionalMooringLine optional_mooring_line(HYDRO_MOOR_PARAMS) { return OptionalMooringLine{{mooring_line(HYDRO_MOOR_ARGS), 0.0f}}; }
__device__ __forceinline__ ExtremesTrack extremes_track(HYDRO_EXT_PARAMS) { return ExtremesTrack{{0u, 0u}, extremes, extremes_stride}; }

// The mooring kernel's arguments, then the extremes record's.  `mooring` may be null.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_ext_tiled_kernel(HYDRO_UP_TO_EXT_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   optional_sea_view(HYDRO_SEA_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS), optional_mooring_line(HYDRO_MOOR_ARGS),
                                                   extremes_track(HYDRO_EXT_ARGS), NoTether{});
}

// hydro_extremes_reset: the empty record, or (st != nullptr) the record of the one sample `st`.
__global__ void __launch_bounds__(kBlock) extremes_reset_kernel(const float* st, uint32_t st_stride, float* ext, uint32_t ext_stride, uint32_t n)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const float inf = __builtin_inff();
    float v[HYDRO_EXT_FIELDS] = {inf, -inf, inf, -inf, inf, -inf, 0.0f, 0.0f};
    if (st) {                                                            // (a kernel argument: wave-uniform)
        const float* r = st + (size_t)tile * st_stride;
#pragma unroll
        for (int a = 0; a < 3; ++a) v[2 * a] = v[2 * a + 1] = *at<float>(r, lane4, a * 256u);
        const float vx = *at<float>(r, lane4, 7 * 256u), vy = *at<float>(r, lane4, 8 * 256u), vz = *at<float>(r, lane4, 9 * 256u);
        v[6] = __builtin_fmaf(vz, vz, __builtin_fmaf(vy, vy, vx * vx));
    }
    store_record<HYDRO_EXT_FIELDS, false>(ext + (size_t)tile * ext_stride, lane4, v);
}

// --------------------------------------------------------------------------
// TETHERS in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_teth): ONE tension-only line between two bodies
// of the same tile - a spring and a damper along the line that never push.  The first term of the model that couples two
// bodies.  Per body a tiled 7-field record ([tiles][7][64], addressed like the mooring record):
//   b(3) | L0 | k | c | partner
// include/hydro.h states the model and the order of operations ("Tether"); tether_wrench below is its ONLY implementation
// (the step kernel and hydro_tether_wrench's kernel both call it).  The line sees the TRUE state and adds its wrench behind
// the mooring line's, in front of the integrator: one fp32 add per component.
//   the exchange: a tile is one wavefront that steps in lockstep, so the partner's fairlead (position P, velocity U) of THIS
//                 step is in the partner lane's registers: six ds_bpermute_b32 hand it over, with no LDS allocation and no
//                 memory traffic.  `partner` is a lane index, never an address: (int)partner & 63, times four, is all the
//                 instruction sees, and a lane that is masked off answers +0.  Every lane that reaches the exchange takes
//                 part in it, tethered or not - the only branch in front of it is the wave-uniform skip.
//   the record  : the extremes kernels stand at 165 VGPRs of 168 and their LDS fills the CU at three blocks, so the seven
//                 values are neither carried through the loop nor parked: every step reads them anew from the caller's
//                 buffer (seven coalesced loads of a launch-invariant 1 792 B per wave, L2 hits after the first step).  The
//                 address is lane4 + the tile's record, a wave-uniform pointer in two SGPRs that an empty asm makes opaque
//                 in every step (LaneSlots::parked's way), so that the compiler neither hoists the loads across the fp64
//                 wrench nor forwards the values through registers.
//   the skip    : a lane has a tether if k > 0 or c > 0.  If no lane of the wavefront has one (ballot == 0) the wave branches
//                 round the evaluation: an untethered tile pays two loads, two compares and the branch
//   no +0       : a lane whose line adds nothing (no tether, slack, or a tension that is not > 0) leaves f6 untouched
//   antisymmetry: negation is exact, so the partner forms -e and -dU, hence the same l2, inv, x, rate and T, and -F, bit for bit
// --------------------------------------------------------------------------
__device__ __forceinline__ float from_lane(uint32_t lane_byte, float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)lane_byte, __builtin_bit_cast(int, v)));
}
// W (force at, torque about the body origin, world frame) of the tether whose record is t[j * 64], j = 0 .. 6, on a body in
// state s.  Returns whether the line pulls; W and `tension` are meaningful (and complete) only then.  To be called in
// wave-uniform control flow by every lane whose partner may ask for its fairlead.
__device__ __forceinline__ bool tether_wrench(const float* t, const float (&s)[HYDRO_STATE_FIELDS], float (&W)[HYDRO_WRENCH_FIELDS], float& tension)
{
    const float k = t[4 * 64], c = t[5 * 64];
    const bool has_tether = k > 0.0f || c > 0.0f;
    if (__builtin_amdgcn_ballot_w64(has_tether) == 0) return false;       // (scalar branch: nobody in this wave is tethered)
    const auto [r00, r01, r02, r10, r11, r12, r20, r21, r22] = rotation_of(s[3], s[4], s[5], s[6]);
    const float bx = t[0 * 64], by = t[1 * 64], bz = t[2 * 64];
    const float rx = __builtin_fmaf(r02, bz, __builtin_fmaf(r01, by, r00 * bx));
    const float ry = __builtin_fmaf(r12, bz, __builtin_fmaf(r11, by, r10 * bx));
    const float rz = __builtin_fmaf(r22, bz, __builtin_fmaf(r21, by, r20 * bx));
    const float px = s[0] + rx, py = s[1] + ry, pz = s[2] + rz;
    const float ux = __builtin_fmaf(s[11], rz, __builtin_fmaf(-s[12], ry, s[7]));
    const float uy = __builtin_fmaf(s[12], rx, __builtin_fmaf(-s[10], rz, s[8]));
    const float uz = __builtin_fmaf(s[10], ry, __builtin_fmaf(-s[11], rx, s[9]));
    const uint32_t partner = ((uint32_t)(int)t[6 * 64] & 63u) << 2;       // (a lane index, in the byte form ds_bpermute takes)
    const float ex = from_lane(partner, px) - px, ey = from_lane(partner, py) - py, ez = from_lane(partner, pz) - pz;
    const float dux = from_lane(partner, ux) - ux, duy = from_lane(partner, uy) - uy, duz = from_lane(partner, uz) - uz;
    const float l2 = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    const float inv = rsqrt_nr(l2);
    const float l = l2 * inv;
    const float x = l - t[3 * 64];
    const float rate = __builtin_fmaf(duz, ez, __builtin_fmaf(duy, ey, dux * ex)) * inv;
    const float cr = c * rate;
    const float T = __builtin_fmaxf(0.0f, __builtin_fmaf(k, x, cr));
    const float ti = T * inv;
    tension = T;
    W[0] = ti * ex; W[1] = ti * ey; W[2] = ti * ez;
    W[3] = __builtin_fmaf(ry, W[2], -(rz * W[1]));
    W[4] = __builtin_fmaf(rz, W[0], -(rx * W[2]));
    W[5] = __builtin_fmaf(rx, W[1], -(ry * W[0]));
    return has_tether && x > 0.0f && T > 0.0f;                            // (l2 = 0: x is NaN, not taut)
}

struct TetherLine {
    using GlobalFloats = const float __attribute__((address_space(1)))*;  // (the empty asm must not cost the loads their address space)
    const float* rec; uint32_t stride;
    GlobalFloats tile_rec; uint32_t lane4;                               // the tile's record: a wave-uniform pointer, in SGPRs
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        tile_rec = (GlobalFloats)(rec + (size_t)tile * stride);
        lane4 = lane4_;
    }
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        GlobalFloats r = tile_rec;
        asm volatile("" : "+s"(r));
        float W[HYDRO_WRENCH_FIELDS], T;
        if (tether_wrench(at<float>((const float*)r, lane4), s, W, T)) {
#pragma unroll
            for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) f6[f] += W[f];
        }
    }
};

// The extremes of the tether kernel: optional (`rec` - a kernel argument: wave-uniform); an absent record loads, updates and
// stores nothing.
struct OptionalExtremesTrack : ExtremesTrack {
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        if (rec) ExtremesTrack::begin(tile, lane4_);
    }
    __device__ __forceinline__ void after_step(const float (&s)[HYDRO_STATE_FIELDS], float T) const
    {
        if (rec) ExtremesTrack::after_step(s, T);
    }
    __device__ __forceinline__ void end(uint32_t tile, uint32_t lane4_) const
    {
        if (rec) ExtremesTrack::end(tile, lane4_);
    }
};
__device__ __forceinline__ OptionalExtremesTrack optional_extremes_track(HYDRO_EXT_PARAMS) { return OptionalExtremesTrack{extremes_track(HYDRO_EXT_ARGS)}; }

// The extremes kernel's arguments, then the tether record's.  `mooring` and `extremes` may be null.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_teth_tiled_kernel(HYDRO_UP_TO_EXT_PARAMS, HYDRO_TETH_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_UP_TO_EXT_OPTIONAL, TetherLine{HYDRO_TETH_ARGS, nullptr, 0u});
}

// --------------------------------------------------------------------------
// TETHER NETS in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_net): `layers` tether records, one behind
// the other ([tiles][7 * layers][64], layer l in rows 7 l .. 7 l + 6), each a complete record of the kind above - so a body
// has up to `layers` lines, and a chain 0-1-2-3-4 is two layers: (0,1) (2,3) | (1,2) (3,4).  include/hydro.h states the
// contract ("Tether net").  Every line is tether_wrench's, from the TRUE state the step starts from, and the wrenches are
// added to f6 in ascending layer order, one fp32 add per component, where the line pulls - one layer gives TetherLine's bits.
//   the loop    : a REAL loop over the layers, never unrolled.  The _teth kernels stand at 163-167 VGPRs of 168: rolled,
//                 the peak pressure is that of one evaluation (plus the trip counter, in SGPRs); unrolled, the compiler
//                 would carry rotation_of(q) and the fairlead arithmetic it shares from layer to layer.  The trip count is
//                 a kernel argument: wave-uniform, so the exchange of every taken layer stays in wave-uniform control
//                 flow and every live lane takes part in its six ds_bpermute_b32.
//   the record  : each trip moves the tile's wave-uniform pointer on by 448 floats and makes it opaque again (TetherLine's
//                 empty asm), so no layer's loads are hoisted or shared.  The quaternion is made opaque per trip in the same
//                 way (four VGPR copies), or the compiler forms rotation_of(q) once in front of the loop.
//   the skip    : per layer, tether_wrench's own ballot: a tile with no line in a layer pays two loads, two compares and the
//                 branch for that layer
// --------------------------------------------------------------------------
struct TetherNet {
    using GlobalFloats = const float __attribute__((address_space(1)))*;
    const float* rec; uint32_t stride, layers;
    GlobalFloats tile_rec; uint32_t lane4;                               // layer 0 of the tile's record: a wave-uniform pointer, in SGPRs
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        tile_rec = (GlobalFloats)(rec + (size_t)tile * stride);
        lane4 = lane4_;
    }
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        GlobalFloats r = tile_rec;
#pragma clang loop unroll(disable)
        for (uint32_t l = 0; l < layers; ++l, r += HYDRO_TETH_FIELDS * HYDRO_TILE) {
            asm volatile("" : "+s"(r));
            // (the orientation as well: rotation_of(q) is the same in every trip, and hoisted in front of the loop it would live
            // across it - nine registers, and paid by a tile without a line)
            float t[HYDRO_STATE_FIELDS];
#pragma unroll
            for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) t[f] = s[f];
            asm volatile("" : "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]));
            float W[HYDRO_WRENCH_FIELDS], T;
            if (tether_wrench(at<float>((const float*)r, lane4), t, W, T)) {
#pragma unroll
                for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) f6[f] += W[f];
            }
        }
    }
};

// The tether kernel's arguments, then the number of layers.  `mooring` and `extremes` may be null.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_net_tiled_kernel(HYDRO_UP_TO_EXT_PARAMS, HYDRO_NET_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_UP_TO_EXT_OPTIONAL, TetherNet{HYDRO_NET_ARGS, nullptr, 0u});
}

// --------------------------------------------------------------------------
// LINK TENSIONS in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_peak): the running maximum of every line's
// tension, per body and layer ([tiles][layers][64] fp32, row l the layer's), updated in every step of a launch.  The states
// between the ends of a launch exist in registers only, so the tensions do too: the design load of a cable - the largest
// tension each link ever carried - can be taken nowhere else.  include/hydro.h states the contract ("Link tensions").
// PeakTetherNet is TetherNet, trip for trip, plus ONE instruction behind the wrench of a line that pulls:
//   the update  : extreme_max(record, T) as a NO-RETURN integer maximum on the bits of T (global_atomic_umax, a vector memory
//                 instruction), from the lanes whose line pulls.  Such a lane has T > 0, and the non-negative floats order as
//                 their bits do as unsigned integers: the larger bits are the larger value, an equal value leaves the slot's
//                 bits, and a NaN already in the slot (bits above +inf's, either sign) stays - extreme_max's rule, bit for bit,
//                 for a record that holds what the entry itself leaves there: +0, a positive value or a NaN.  A NaN sample has no
//                 T > 0 and never gets here.
//   why not load, compare, store: the _net kernels stand at 163-167 VGPRs of 168 and their LDS fills the CU at three blocks, so
//                 the accumulators can be neither carried nor parked.  Read-modify-write in the caller's buffer would put a
//                 load's round trip to L2 into every taken layer of every step and cost a register for the value; the
//                 maximum is done by the L2 itself, nothing comes back and the wave does not wait.  Each slot belongs to one
//                 lane of one wave: there is no contention, the atomic is used for where it executes, not for mutual exclusion.
//   the slot    : the tile's row of the record, a wave-uniform pointer in two SGPRs that moves on by 64 floats per trip and is
//                 made opaque per trip like the net's, plus lane4: the compiler forms the 64-bit address with one
//                 v_lshl_add_u64 inside the branch (an atomic takes no scalar base here), in registers that are free there.
//                 Left transparent, the address is formed in front of the step loop and lives across it: 12 bytes of scratch
//                 in the eight instantiations that stand at 167
//   control flow: the update sits behind tether_wrench, inside the branch of the lanes whose line pulls: the exchange of every
//                 taken layer is in wave-uniform control flow as in TetherNet, and a tile without a line in a layer branches
//                 round everything on tether_wrench's ballot and touches no memory
// Nothing read here feeds back: state, prev_out, energy, log and extremes are TetherNet's bits.
// --------------------------------------------------------------------------
struct PeakTetherNet : TetherNet {
    using GlobalWords = uint32_t __attribute__((address_space(1)))*;
    float* peaks; uint32_t peaks_stride;
    GlobalWords tile_peaks;                                              // row 0 of the tile's record: a wave-uniform pointer, in SGPRs
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        TetherNet::begin(tile, lane4_);
        tile_peaks = (GlobalWords)(peaks + (size_t)tile * peaks_stride);
    }
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        GlobalFloats r = tile_rec;
        GlobalWords p = tile_peaks;
#pragma clang loop unroll(disable)
        for (uint32_t l = 0; l < layers; ++l, r += HYDRO_TETH_FIELDS * HYDRO_TILE, p += HYDRO_TILE) {
            asm volatile("" : "+s"(r), "+s"(p));                         // (p as well: left alone, the lane's 64-bit slot address is formed in front of the step loop and lives across it)
            float t[HYDRO_STATE_FIELDS];
#pragma unroll
            for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) t[f] = s[f];
            asm volatile("" : "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]));
            float W[HYDRO_WRENCH_FIELDS], T;
            if (tether_wrench(at<float>((const float*)r, lane4), t, W, T)) {
#pragma unroll
                for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) f6[f] += W[f];
                (void)__hip_atomic_fetch_max(at<uint32_t>((uint32_t*)p, lane4), __builtin_bit_cast(uint32_t, T), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
};

// The net kernel's arguments, then the record of the link tensions.  `mooring` and `extremes` may be null.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_peak_tiled_kernel(HYDRO_UP_TO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_UP_TO_EXT_OPTIONAL, PeakTetherNet{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr});
}

// --------------------------------------------------------------------------
// MOORING SPREADS in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_spread): `layers` mooring records, one
// behind the other ([tiles][9 * layers][64], layer l in rows 9 l .. 9 l + 8), each a complete record of MooringLine's kind -
// so a body has up to `layers` anchored lines, the three or four of a spread mooring.  include/hydro.h states the contract
// ("Mooring spread").  Every line is mooring_wrench's, from the TRUE state the step starts from, and the wrenches are added
// to f6 in ascending layer order behind the bed and in front of the tethers, one fp32 add per component, where the line
// pulls - one layer gives OptionalMooringLine's bits.  TetherNet's design (above), applied to the anchored line:
//   the loop    : a REAL loop over the layers, never unrolled: the peak pressure is that of one evaluation plus the fold.
//                 The trip count is a kernel argument, wave-uniform
//   the record  : NOT parked.  Four layers are 36 KB of LDS per block and the _peak kernels' LDS fills the CU at three blocks
//                 as it is, so every trip reads its nine values from the caller's buffer (launch-invariant, L2 hits after
//                 the first step): the tile's wave-uniform pointer moves on by 576 floats per trip and is made opaque
//                 again, so no layer's loads are hoisted or shared; the quaternion likewise, so that rotation_of stays
//                 behind the layer's ballot.  This family's LDS is the _peak kernels' less the line's nine slots
//   the skip    : per layer, mooring_wrench's own ballot: a tile with no line in a layer pays two loads, two compares and
//                 the branch for that layer
//   the tension : what the extremes record takes is the LARGEST tension of any of the body's lines in the step, folded from
//                 +0 over the layers in ascending order by extreme_max(acc, pulls ? T : +0) - TrackedMooringLine's value for
//                 one layer, bit for bit
// A null record evaluates nothing and reports +0.
// --------------------------------------------------------------------------
struct MooringSpread {
    using GlobalFloats = const float __attribute__((address_space(1)))*;
    const float* rec; uint32_t stride, layers;
    GlobalFloats tile_rec; uint32_t lane4;                               // layer 0 of the tile's record: a wave-uniform pointer, in SGPRs
    mutable float last;
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        tile_rec = (GlobalFloats)(rec + (size_t)tile * stride);
        lane4 = lane4_;
    }
    __device__ __forceinline__ void end(float (&d)[3]) const             // (MooringLine::end's, for the same reason)
    {
        asm volatile("" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]));
    }
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        float acc = 0.0f;
        if (rec) {                                                       // (a kernel argument: wave-uniform)
            GlobalFloats r = tile_rec;
#pragma clang loop unroll(disable)
            for (uint32_t l = 0; l < layers; ++l, r += HYDRO_MOOR_FIELDS * HYDRO_TILE) {
                asm volatile("" : "+s"(r));
                float t[HYDRO_STATE_FIELDS];
#pragma unroll
                for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) t[f] = s[f];
                asm volatile("" : "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]));
                float W[HYDRO_WRENCH_FIELDS], T = 0.0f;
                const bool pulls = mooring_wrench(at<float>((const float*)r, lane4), t, W, T);
                if (pulls) {
#pragma unroll
                    for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) f6[f] += W[f];
                }
                acc = extreme_max(acc, pulls ? T : 0.0f);
            }
        }
        last = acc;
    }
    __device__ __forceinline__ float tension() const { return last; }
};
__device__ __forceinline__ MooringSpread mooring_spread(HYDRO_SPREAD_PARAMS) { return MooringSpread{HYDRO_SPREAD_ARGS, nullptr, 0u, 0.0f}; }

// The net and the link tensions of the spread kernel: each optional.  No net is a net of no layers (the launch says so); no
// record of link tensions (`peaks` - a kernel argument: wave-uniform) is TetherNet's loop, which touches no memory but the net.
struct OptionalPeakTetherNet : PeakTetherNet {
    __device__ __forceinline__ void add(const float (&s)[HYDRO_STATE_FIELDS], float (&f6)[HYDRO_WRENCH_FIELDS]) const
    {
        if (peaks) PeakTetherNet::add(s, f6);
        else TetherNet::add(s, f6);
    }
};

// The _peak kernel's arguments with the number of mooring layers behind the mooring record's stride.  Everything but
// `mooring` may be null.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_spread_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                    HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_SPREAD_PARAMS,
                                                                                                    HYDRO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   optional_sea_view(HYDRO_SEA_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS), mooring_spread(HYDRO_SPREAD_ARGS),
                                                   optional_extremes_track(HYDRO_EXT_ARGS),
                                                   OptionalPeakTetherNet{{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr}});
}

// --------------------------------------------------------------------------
// IRREGULAR SEAS in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_irr): the sea state's model with up to
// HYDRO_SPECTRUM_WAVES_MAX components - a JONSWAP or Pierson-Moskowitz spectrum cut into bins (hydro_set_sea_spectrum;
// include/hydro.h, "Sea spectrum").  spectrum_water below is its ONLY implementation (the step kernel and
// hydro_sea_spectrum_sample's kernel both call it), and for up to HYDRO_SEA_WAVES_MAX components it returns sea_water's bits:
// the same statements on the same inputs, the sums in ascending component order, eta from +0 and u from U.
//   the loop   : a REAL loop over the components, unrolled in groups of four so that a group's scalar loads are in flight
//                together (one wait per group; the remainder runs one by one): cs[] and sn[] of sea_water are 128 registers at
//                64 components, so nothing is kept per component.  The second pass needs all of eta before any exp, and forms
//                th_j, its reduction and its cosine AGAIN - the same instructions on the same inputs, hence the same bits as
//                the first pass (tau_j is recomputed with them: the fp64 chain is wave-uniform and short)
//   the lanes  : every lane evaluates every component.  Dead lanes of a partial tile never reach a sea policy
//                (fused_multi_body), so no lane may compute a phase for another
//   the table  : SeaTable's header and records, 16 + 64 * 48 = 3088 B, read through the CONSTANT address space with a
//                wave-uniform index: scalar loads in every trip, no vector register holds a component between trips
// --------------------------------------------------------------------------
struct SpectrumTable {
    float u[3]; uint32_t waves;
    SeaWave w[HYDRO_SPECTRUM_WAVES_MAX];
};
typedef const __attribute__((address_space(4))) SpectrumTable* SpectrumTablePtr;
typedef const __attribute__((address_space(4))) SeaWave* SeaWavePtr;

// r_j of include/hydro.h for component `w` at time t: th_j in revolutions, reduced to [-1/2, 1/2] - sea_water's statements.
__device__ __forceinline__ float spectrum_revolutions(SeaWavePtr w, double t, float px, float py)
{
    constexpr double kInv2Pi = 0.15915494309189535, kTwoPiHi = 6.283185307179586, kTwoPiLo = 2.4492935982947064e-16;
    const double x = __builtin_fma(-w->omega, t, w->phi);
    const double m = __builtin_rint(x * kInv2Pi);
    const float tau = (float)__builtin_fma(-m, kTwoPiLo, __builtin_fma(-m, kTwoPiHi, x));
    const float th = __builtin_fmaf(w->kx, px, __builtin_fmaf(w->ky, py, tau));
    const float rev = th * 0.15915494309189535f;
    return rev - __builtin_rintf(rev);
}

// eta and u of the water at (px, py) for a body whose centre is at pz, at the start of step `step`: sea_water for any number
// of components.
__device__ __forceinline__ void spectrum_water(SpectrumTablePtr tab, uint32_t waves, int64_t step, double dt, float px, float py, float pz,
                                               float& eta, float (&u)[3])
{
    const double t = (double)step * dt;
    eta = 0.0f;
#pragma clang loop unroll_count(4)
    for (uint32_t j = 0; j < waves; ++j) {                   // (wave-uniform)
        const float r = spectrum_revolutions(&tab->w[j], t, px, py);
        eta = __builtin_fmaf(tab->w[j].a, __builtin_amdgcn_cosf(r), eta);
    }
    const float zc = __builtin_fminf(pz - eta, 0.0f);
    u[0] = tab->u[0]; u[1] = tab->u[1]; u[2] = tab->u[2];
#pragma clang loop unroll_count(4)
    for (uint32_t j = 0; j < waves; ++j) {
        const float r = spectrum_revolutions(&tab->w[j], t, px, py);
        const float cs = __builtin_amdgcn_cosf(r), sn = __builtin_amdgcn_sinf(r);
        const float e = __builtin_amdgcn_exp2f(tab->w[j].kl2 * zc);
        const float ec = e * cs, es = e * sn;
        u[0] = __builtin_fmaf(tab->w[j].cx, ec, u[0]);
        u[1] = __builtin_fmaf(tab->w[j].cy, ec, u[1]);
        u[2] = __builtin_fmaf(tab->w[j].aw, es, u[2]);
    }
}

// SeaView with spectrum_water for the water: the same seven values parked in the same slots (the two never meet in a
// kernel), the same restore.  Not optional: the host launches the kernel below only while a spectrum is set.
struct SpectrumView : SeaView {
    __device__ __forceinline__ void view(uint32_t k, float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS]) const
    {
        float eta, u[3];
        spectrum_water((SpectrumTablePtr)tab, waves, step0 + (int64_t)k, dt, s[0], s[1], s[2], eta, u);
        float* m = parked();
        m[0] = s[2];
        s[2] = s[2] - eta;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            m[(1 + i) * 64] = s[7 + i];
            m[(4 + i) * 64] = pv[i];
            s[7 + i] = s[7 + i] - u[i];
            pv[i] = pv[i] - u[i];
        }
    }
};
__device__ __forceinline__ SpectrumView spectrum_view(HYDRO_SEA_PARAMS) { return SpectrumView{sea_view(HYDRO_SEA_ARGS)}; }

// The _spread kernel's arguments, unchanged; the sea group carries the spectrum's table and count.  Everything else may be null.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_irr_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                 HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_SPREAD_PARAMS,
                                                                                                 HYDRO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   spectrum_view(HYDRO_SEA_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS), mooring_spread(HYDRO_SPREAD_ARGS),
                                                   optional_extremes_track(HYDRO_EXT_ARGS),
                                                   OptionalPeakTetherNet{{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr}});
}

// hydro_sea_spectrum_sample: sea_sample_kernel against the spectrum.
__global__ void __launch_bounds__(kBlock) spectrum_sample_kernel(const float* st, uint32_t st_stride, float* out, uint32_t out_stride, uint32_t n,
                                                                 const void* sea_table, uint32_t sea_waves, int64_t step, double sea_dt)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const float* r = st + (size_t)tile * st_stride;
    float eta, u[3];
    spectrum_water((SpectrumTablePtr)sea_table, sea_waves, step, sea_dt, *at<float>(r, lane4, 0u), *at<float>(r, lane4, 256u), *at<float>(r, lane4, 512u), eta, u);
    const float o[HYDRO_SEA_FIELDS] = {eta, u[0], u[1], u[2]};
    store_record<HYDRO_SEA_FIELDS, false>(out + (size_t)tile * out_stride, lane4, o);
}

// --------------------------------------------------------------------------
// RESPONSE STATISTICS in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_stat): what a mooring designer reads
// off an irregular-sea run besides the peak - per body and for two channels the sum and the sum of squares of the response
// about a reference level, and the number of times it crossed that level upwards (include/hydro.h, "Statistics", states the
// sample, the arithmetic and the record).  Like the extremes the record is READ at the start of a launch and WRITTEN at its
// end, so it accumulates across launches until hydro_statistics_reset.
//   the slot    : the policy WRAPS OptionalExtremesTrack in the extremes slot of fused_multi_body: begin / after_step / end
//                 call the extremes' own and then their own, so fused_multi_body and every existing kernel stay as they are
//   the sample  : the extremes' - the state the step produced and the tension moor.tension() handed over.  The two channels
//                 are kernel arguments (wave-uniform): a channel's value is picked by scalar compares, v_cndmask at most
//   the record  : four doubles and two words per lane.  The _spread and _irr kernels stand at 156-163 VGPRs of 168, so they
//                 are not carried through the loop: each lane parks them in LDS, [wave][10][64] floats - a double as two
//                 planes, low word then high word, so that lane4 addresses them like every parked float (10 240 B per
//                 block; LaneSlots' way, with the extremes' lane4 and wave offset: the loop keeps no register for this
//                 policy's address) - and reads, updates and writes them behind the integrator.  43 008 + 10 240 = 53 248 B
//                 per block: three blocks fit a CU
//   the levels  : NOT parked.  Two floats per lane from the caller's buffer in every step, through the tile's wave-uniform
//                 pointer made opaque in every step (MooringSpread's way): launch-invariant, L2 hits after the first step
//   the sums    : fp64, one rounding per operation, NO fma: d = x - L, S1 += d, q = d * d, S2 += q.  The empty asm on q
//                 stands between the product and the sum, so that no contraction can join them
//   the words   : bit 31 = "the last sample was not above its level", bits 0 .. 30 the count (hydro.h states the update)
//   n           : not touched in the loop: end() adds `steps` to the word it reads from the caller's record
// Nothing the policy computes feeds back: state, prev_out, energy, log, extremes and link tensions are the wrapped kernel's bits.
// --------------------------------------------------------------------------
#define HYDRO_STAT_PARAMS void* statistics, uint32_t statistics_stride, const float* levels, uint32_t levels_stride,             \
                          uint32_t channel_a, uint32_t channel_b
#define HYDRO_STAT_ARGS statistics, statistics_stride, levels, levels_stride, channel_a, channel_b
constexpr uint32_t kStatSlots = 10;                                      // four doubles as eight half planes, two words
constexpr uint32_t kStatWordsAt = 4u * 512u;                             // the words behind the sums in the caller's record

struct StatisticsTrack : OptionalExtremesTrack {
    using GlobalFloats = const float __attribute__((address_space(1)))*;
    using GlobalBytes = char __attribute__((address_space(1)))*;
    void* stat; uint32_t stat_stride; const float* lev; uint32_t lev_stride, ch_a, ch_b, steps;
    GlobalFloats tile_lev; GlobalBytes tile_stat;                        // the tile's two records: wave-uniform pointers, in SGPRs
    static __device__ __forceinline__ float* slots()
    {
        __shared__ __attribute__((aligned(16))) float lds[kBlock * kStatSlots];
        return lds;
    }
    // The lane's slot 0, [wave][10][64] floats: the extremes' lane4 and wave offset serve (begin sets both, whether or not there
    // is an extremes record) - 10 / 8 of that offset is this policy's, in two scalar instructions, and no register of its own.
    __device__ __forceinline__ float* parked() const
    {
        uint32_t w_off = wave_off;
        asm volatile("" : "+s"(w_off));
        return at<float>(slots(), lane4 + (w_off >> 3) * kStatSlots);
    }
    // a parked double: its low word in plane 2 j, its high word in plane 2 j + 1
    static __device__ __forceinline__ double parked_double(const float* m, uint32_t j)
    {
        return __hiloint2double(__builtin_bit_cast(int, m[(2u * j + 1u) * 64u]), __builtin_bit_cast(int, m[(2u * j) * 64u]));
    }
    static __device__ __forceinline__ void park_double(float* m, uint32_t j, double v)
    {
        m[(2u * j) * 64u] = __builtin_bit_cast(float, __double2loint(v));
        m[(2u * j + 1u) * 64u] = __builtin_bit_cast(float, __double2hiint(v));
    }
    // the sample of channel `ch` (wave-uniform): s[0..2], s[7..9] or the tension
    static __device__ __forceinline__ float sample(uint32_t ch, const float (&s)[HYDRO_STATE_FIELDS], float T)
    {
        float x = T;
        x = ch == HYDRO_STAT_X ? s[0] : x;
        x = ch == HYDRO_STAT_Y ? s[1] : x;
        x = ch == HYDRO_STAT_Z ? s[2] : x;
        x = ch == HYDRO_STAT_VX ? s[7] : x;
        x = ch == HYDRO_STAT_VY ? s[8] : x;
        x = ch == HYDRO_STAT_VZ ? s[9] : x;
        return x;
    }
    // one sample x of slot c (0: a, 1: b) against its level L
    static __device__ __forceinline__ void fold(float* m, uint32_t c, float x, float L)
    {
        const double d = (double)x - (double)L;
        park_double(m, 2u * c, parked_double(m, 2u * c) + d);
        double q = d * d;
        asm volatile("" : "+v"(q));                                      // (no fma: the product is rounded before the sum sees it)
        park_double(m, 2u * c + 1u, parked_double(m, 2u * c + 1u) + q);
        const bool above = x > L;                                        // (false for a NaN)
        const uint32_t w = __builtin_bit_cast(uint32_t, m[(8u + c) * 64u]);
        m[(8u + c) * 64u] = __builtin_bit_cast(float, ((w + ((w >> 31) & (above ? 1u : 0u))) & 0x7fffffffu) | (above ? 0u : 0x80000000u));
    }
    __device__ __forceinline__ void begin(uint32_t tile, uint32_t lane4_)
    {
        OptionalExtremesTrack::begin(tile, lane4_);
        lane4 = lane4_;                                                  // (what ExtremesTrack::claim sets, also without an extremes record)
        wave_off = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * (kExtSlots * 256u);
        tile_lev = (GlobalFloats)(lev + (size_t)tile * lev_stride);
        tile_stat = (GlobalBytes)(reinterpret_cast<float*>(stat) + (size_t)tile * stat_stride);
        float* m = at<float>(slots(), lane4 + (wave_off >> 3) * kStatSlots);
        const char* r = (const char*)tile_stat;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) park_double(m, j, *at<double>(r, lane4 * 2u, j * 512u));
#pragma unroll
        for (uint32_t c = 0; c < 2u; ++c) m[(8u + c) * 64u] = *at<float>(r, lane4, kStatWordsAt + c * 256u);
    }
    __device__ __forceinline__ void after_step(const float (&s)[HYDRO_STATE_FIELDS], float T) const
    {
        OptionalExtremesTrack::after_step(s, T);
        GlobalFloats L = tile_lev;
        asm volatile("" : "+s"(L));
        const float la = *at<float>((const float*)L, lane4, 0u), lb = *at<float>((const float*)L, lane4, 256u);
        float* m = parked();
        fold(m, 0u, sample(ch_a, s, T), la);
        fold(m, 1u, sample(ch_b, s, T), lb);
    }
    // Only live lanes come here (fused_multi_body): the padding lanes of the last tile are never written.
    __device__ __forceinline__ void end(uint32_t tile, uint32_t lane4_) const
    {
        OptionalExtremesTrack::end(tile, lane4_);
        const float* m = parked();
        char* r = (char*)tile_stat;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) *at<double>(r, lane4_ * 2u, j * 512u) = parked_double(m, j);
#pragma unroll
        for (uint32_t c = 0; c < 2u; ++c) *at<float>(r, lane4_, kStatWordsAt + c * 256u) = m[(8u + c) * 64u];
        uint32_t* count = at<uint32_t>(r, lane4_, kStatWordsAt + 2u * 256u);
        *count = *count + steps;
    }
};
__device__ __forceinline__ StatisticsTrack statistics_track(HYDRO_EXT_PARAMS, HYDRO_STAT_PARAMS, uint32_t steps)
{
    return StatisticsTrack{optional_extremes_track(HYDRO_EXT_ARGS), statistics, statistics_stride, levels, levels_stride, channel_a, channel_b, steps, nullptr, nullptr};
}

// The _spread kernel's arguments, then the statistics group.  Everything in front of the group may be null; `statistics` and `levels` may not.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_stat_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                  HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_SPREAD_PARAMS,
                                                                                                  HYDRO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS, HYDRO_STAT_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   optional_sea_view(HYDRO_SEA_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS), mooring_spread(HYDRO_SPREAD_ARGS),
                                                   statistics_track(HYDRO_EXT_ARGS, HYDRO_STAT_ARGS, steps),
                                                   OptionalPeakTetherNet{{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr}});
}

// The same through the sea spectrum: the _irr kernel's arguments, then the statistics group.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_irr_stat_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                      HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_SPREAD_PARAMS,
                                                                                                      HYDRO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS, HYDRO_STAT_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   spectrum_view(HYDRO_SEA_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS), mooring_spread(HYDRO_SPREAD_ARGS),
                                                   statistics_track(HYDRO_EXT_ARGS, HYDRO_STAT_ARGS, steps),
                                                   OptionalPeakTetherNet{{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr}});
}

// --------------------------------------------------------------------------
// SEA ENSEMBLES in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_ens): `count` spectra of the model above,
// one SpectrumTable behind the other in an engine-owned device table, and block m of `tiles_per_sea` tiles steps through
// member m (hydro_set_sea_ensemble; include/hydro.h, "Sea ensemble").  The water is spectrum_water's, statement for
// statement: the ONLY thing an ensemble changes is where the wave's table pointer points.
//   the member : tile / tiles_per_sea, formed ONCE in begin from the wave's tile (wave-uniform, told to the compiler with
//                v_readfirstlane) - four waves of a block may read four different members (tiles_per_sea = 1)
//   the pointer: SeaView::tab moved on by member * sizeof(SpectrumTable): a scalar 64-bit add in front of the step loop.
//                The component loops read through it with scalar loads as before; nothing new is live in the step loop
//   dead waves : a wave whose lanes are all >= n never reaches a sea policy (fused_multi_body), so a member index past
//                `count` is never formed into an address that is read: the host refuses a launch whose LIVE tiles need more
//                members than the table holds
// view and restore are SpectrumView's; fused_multi_body is not touched.
// --------------------------------------------------------------------------
#define HYDRO_ENS_PARAMS uint32_t tiles_per_sea
#define HYDRO_ENS_ARGS tiles_per_sea
// the table of the member that `tile` steps through (both wave-uniform)
__device__ __forceinline__ SpectrumTablePtr ensemble_member(SpectrumTablePtr table, uint32_t tile, uint32_t tiles_per_sea)
{
    // (there is no scalar divide: the quotient of two scalars is formed with vector instructions whichever way it is written.  Left
    // to itself the compiler fails on it here ("illegal VGPR to SGPR copy" in every instantiation), so both operands are handed
    // over as vector values, the quotient is taken as one, and it comes back through v_readfirstlane like wave_tile's index)
    uint32_t t = tile, d = tiles_per_sea;
    asm volatile("" : "+v"(t), "+v"(d));
    uint32_t q = t / d;
    asm volatile("" : "+v"(q));
    return table + __builtin_amdgcn_readfirstlane(q);
}
struct SpectrumEnsembleView : SpectrumView {
    uint32_t tiles_per_sea;
    __device__ __forceinline__ void begin(uint32_t lane4_)
    {
        SpectrumView::begin(lane4_);
        tab = (SeaTablePtr)ensemble_member((SpectrumTablePtr)tab, wave_tile<kBlock>(blockIdx.x), tiles_per_sea);
    }
};
__device__ __forceinline__ SpectrumEnsembleView spectrum_ensemble_view(HYDRO_SEA_PARAMS, HYDRO_ENS_PARAMS)
{
    return SpectrumEnsembleView{spectrum_view(HYDRO_SEA_ARGS), HYDRO_ENS_ARGS};
}

// The _irr kernel's arguments, then the ensemble's; the sea group carries the ensemble's table and the members' count of components.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_ens_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                 HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_SPREAD_PARAMS,
                                                                                                 HYDRO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS, HYDRO_ENS_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   spectrum_ensemble_view(HYDRO_SEA_ARGS, HYDRO_ENS_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS),
                                                   mooring_spread(HYDRO_SPREAD_ARGS), optional_extremes_track(HYDRO_EXT_ARGS),
                                                   OptionalPeakTetherNet{{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr}});
}

// The _irr_stat kernel's arguments, then the ensemble's.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_ens_stat_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                      HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_SPREAD_PARAMS,
                                                                                                      HYDRO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS, HYDRO_STAT_PARAMS,
                                                                                                      HYDRO_ENS_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   spectrum_ensemble_view(HYDRO_SEA_ARGS, HYDRO_ENS_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS),
                                                   mooring_spread(HYDRO_SPREAD_ARGS), statistics_track(HYDRO_EXT_ARGS, HYDRO_STAT_ARGS, steps),
                                                   OptionalPeakTetherNet{{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr}});
}

// hydro_sea_ensemble_sample: spectrum_sample_kernel with every tile read against its member.
__global__ void __launch_bounds__(kBlock) ensemble_sample_kernel(const float* st, uint32_t st_stride, float* out, uint32_t out_stride, uint32_t n,
                                                                 const void* sea_table, uint32_t sea_waves, int64_t step, double sea_dt, HYDRO_ENS_PARAMS)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const float* r = st + (size_t)tile * st_stride;
    float eta, u[3];
    spectrum_water(ensemble_member((SpectrumTablePtr)sea_table, tile, tiles_per_sea), sea_waves, step, sea_dt, *at<float>(r, lane4, 0u), *at<float>(r, lane4, 256u),
                   *at<float>(r, lane4, 512u), eta, u);
    const float o[HYDRO_SEA_FIELDS] = {eta, u[0], u[1], u[2]};
    store_record<HYDRO_SEA_FIELDS, false>(out + (size_t)tile * out_stride, lane4, o);
}

// --------------------------------------------------------------------------
// FINITE-DEPTH SEAS in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_fd): the ensemble's spectra in water of
// still-water depth h, where the orbital velocity goes with cosh / sinh of the height above the bed instead of e^{kappa z}
// (hydro_set_sea_finite_depth; include/hydro.h, "Finite-depth sea").  depth_water below is its ONLY implementation (the step
// kernels and hydro_sea_finite_depth_sample's kernel both call it): spectrum_water with a second exponential per component.
//   the record : SeaWave stays at 48 B - `pad` holds gl_j = -2 kappa_j h log2(e), and cx, cy, aw arrive already divided by
//                1 - e^{-2 kappa_j h} (the host, in fp64).  The table has SpectrumTable's layout but is one of its own: the deep
//                kernels never see scaled constants
//   the profile: E = exp2(kl2 zc), G = exp2(gl - kl2 zc): (E + G) / (1 - q) = cosh(kappa (zc + h)) / sinh(kappa h) under the
//                horizontal velocity, (E - G) / (1 - q) = sinh(..) / sinh(kappa h) under the vertical one.  One more v_exp_f32,
//                one fma, an add and a subtract per component; nothing more is loaded
//   the clamp  : zc = max(min(z_rel, 0), -h) - nothing below the bed, and zc is finite whatever p_z is.  -h is ONE kernel
//                argument (HYDRO_FD_PARAMS), wave-uniform
//   deep water : with q_j = 0 and G = 0 (kappa_j h beyond a few hundred) every statement returns spectrum_water's bits
// The first pass, spectrum_revolutions and the member's table pointer are the ensemble's; a lone spectrum is an ensemble of one.
// --------------------------------------------------------------------------
#define HYDRO_FD_PARAMS float neg_depth
#define HYDRO_FD_ARGS neg_depth
__device__ __forceinline__ void depth_water(SpectrumTablePtr tab, uint32_t waves, int64_t step, double dt, float px, float py, float pz, HYDRO_FD_PARAMS,
                                            float& eta, float (&u)[3])
{
    const double t = (double)step * dt;
    eta = 0.0f;
#pragma clang loop unroll_count(4)
    for (uint32_t j = 0; j < waves; ++j) {                   // (wave-uniform)
        const float r = spectrum_revolutions(&tab->w[j], t, px, py);
        eta = __builtin_fmaf(tab->w[j].a, __builtin_amdgcn_cosf(r), eta);
    }
    const float zc = __builtin_fmaxf(__builtin_fminf(pz - eta, 0.0f), neg_depth);
    u[0] = tab->u[0]; u[1] = tab->u[1]; u[2] = tab->u[2];
#pragma clang loop unroll_count(4)
    for (uint32_t j = 0; j < waves; ++j) {
        const float r = spectrum_revolutions(&tab->w[j], t, px, py);
        const float cs = __builtin_amdgcn_cosf(r), sn = __builtin_amdgcn_sinf(r);
        const float e = __builtin_amdgcn_exp2f(tab->w[j].kl2 * zc);
        const float g = __builtin_amdgcn_exp2f(__builtin_fmaf(-tab->w[j].kl2, zc, tab->w[j].pad));
        const float ec = (e + g) * cs, es = (e - g) * sn;
        u[0] = __builtin_fmaf(tab->w[j].cx, ec, u[0]);
        u[1] = __builtin_fmaf(tab->w[j].cy, ec, u[1]);
        u[2] = __builtin_fmaf(tab->w[j].aw, es, u[2]);
    }
}

// SpectrumEnsembleView with depth_water for the water: begin (the member's table) and restore are inherited.
struct DepthEnsembleView : SpectrumEnsembleView {
    float neg_depth;
    __device__ __forceinline__ void view(uint32_t k, float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS]) const
    {
        float eta, u[3];
        depth_water((SpectrumTablePtr)tab, waves, step0 + (int64_t)k, dt, s[0], s[1], s[2], HYDRO_FD_ARGS, eta, u);
        float* m = parked();
        m[0] = s[2];
        s[2] = s[2] - eta;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            m[(1 + i) * 64] = s[7 + i];
            m[(4 + i) * 64] = pv[i];
            s[7 + i] = s[7 + i] - u[i];
            pv[i] = pv[i] - u[i];
        }
    }
};
__device__ __forceinline__ DepthEnsembleView depth_ensemble_view(HYDRO_SEA_PARAMS, HYDRO_ENS_PARAMS, HYDRO_FD_PARAMS)
{
    return DepthEnsembleView{spectrum_ensemble_view(HYDRO_SEA_ARGS, HYDRO_ENS_ARGS), HYDRO_FD_ARGS};
}

// The _ens kernel's arguments, then the depth; the sea group carries the finite-depth table and the members' count of components.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_fd_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_SPREAD_PARAMS,
                                                                                                HYDRO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS, HYDRO_ENS_PARAMS,
                                                                                                HYDRO_FD_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   depth_ensemble_view(HYDRO_SEA_ARGS, HYDRO_ENS_ARGS, HYDRO_FD_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS),
                                                   mooring_spread(HYDRO_SPREAD_ARGS), optional_extremes_track(HYDRO_EXT_ARGS),
                                                   OptionalPeakTetherNet{{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr}});
}

// The _ens_stat kernel's arguments, then the depth.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_fd_stat_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                     HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_SPREAD_PARAMS,
                                                                                                     HYDRO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS, HYDRO_STAT_PARAMS,
                                                                                                     HYDRO_ENS_PARAMS, HYDRO_FD_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   depth_ensemble_view(HYDRO_SEA_ARGS, HYDRO_ENS_ARGS, HYDRO_FD_ARGS), optional_seabed_contact(HYDRO_OPT_BED_ARGS),
                                                   mooring_spread(HYDRO_SPREAD_ARGS), statistics_track(HYDRO_EXT_ARGS, HYDRO_STAT_ARGS, steps),
                                                   OptionalPeakTetherNet{{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr}});
}

// hydro_sea_finite_depth_sample: ensemble_sample_kernel calling depth_water.
__global__ void __launch_bounds__(kBlock) depth_sample_kernel(const float* st, uint32_t st_stride, float* out, uint32_t out_stride, uint32_t n,
                                                              const void* sea_table, uint32_t sea_waves, int64_t step, double sea_dt, HYDRO_ENS_PARAMS, HYDRO_FD_PARAMS)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const float* r = st + (size_t)tile * st_stride;
    float eta, u[3];
    depth_water(ensemble_member((SpectrumTablePtr)sea_table, tile, tiles_per_sea), sea_waves, step, sea_dt, *at<float>(r, lane4, 0u), *at<float>(r, lane4, 256u),
                *at<float>(r, lane4, 512u), HYDRO_FD_ARGS, eta, u);
    const float o[HYDRO_SEA_FIELDS] = {eta, u[0], u[1], u[2]};
    store_record<HYDRO_SEA_FIELDS, false>(out + (size_t)tile * out_stride, lane4, o);
}

// --------------------------------------------------------------------------
// A SHEARED CURRENT in the loop of the multi-step kernel (hydro_step_fused_tiled_multi_shear): a scene-wide current profile over
// depth, piecewise linear between up to HYDRO_CURRENT_KNOTS_MAX knots (z_l, V_l), added to the finite-depth sea's water
// (hydro_set_current_profile; include/hydro.h, "Current profile").  sheared_water below is its ONLY implementation (the step
// kernels and hydro_current_profile_sample's kernel both call it): depth_water, UNEDITED, then the knot loop, then one add per
// component.
//   the depth  : zc = max(min(p_z - eta, 0), -h) over again from depth_water's eta - the statement and the inputs of the orbital
//                velocities' zc, hence its bits: the profile rides with the instantaneous surface, and zc is finite for every p_z
//   the loop   : P = V_0, then per segment t = min(max((zc - z_l) * inv_l, 0), 1) and P_i = fma(D_l,i, t, P_i), in ascending l.
//                Branch-free: a segment below the body adds all of D_l, one above it adds +-0 * D_l.  A REAL loop over the
//                segments (wave-uniform count), its values dead once u is formed
//   the table  : a 16-byte header (V_0, the knot count) and 16 records of z_l, inv_l, D_l padded to 32 B: 528 B, engine-owned,
//                read through the CONSTANT address space with a wave-uniform index as the spectrum table is: scalar loads, no
//                LDS staging, no vector register holds a knot between trips
//   the add    : u_i = u_fd,i + P_i behind everything depth_water does; eta, the relative state and restore are the _fd rung's
// The host launches these kernels only while a profile (knots >= 1) AND a finite-depth sea are set.
// --------------------------------------------------------------------------
struct CurrentKnot { float z, inv, d[3], pad[3]; };
struct CurrentTable {
    float v0[3]; uint32_t knots;
    CurrentKnot k[HYDRO_CURRENT_KNOTS_MAX];
};
static_assert(sizeof(CurrentKnot) == 32 && sizeof(CurrentTable) == 16 + 32 * HYDRO_CURRENT_KNOTS_MAX, "the knot table's layout");
typedef const __attribute__((address_space(4))) CurrentTable* CurrentTablePtr;
#define HYDRO_SHEAR_PARAMS const void* knot_table, uint32_t knots
#define HYDRO_SHEAR_ARGS knot_table, knots
__device__ __forceinline__ void sheared_water(SpectrumTablePtr tab, uint32_t waves, int64_t step, double dt, float px, float py, float pz, HYDRO_FD_PARAMS,
                                              CurrentTablePtr prof, uint32_t knots, float& eta, float (&u)[3])
{
    depth_water(tab, waves, step, dt, px, py, pz, HYDRO_FD_ARGS, eta, u);
    const float zc = __builtin_fmaxf(__builtin_fminf(pz - eta, 0.0f), neg_depth);
    float p[3] = {prof->v0[0], prof->v0[1], prof->v0[2]};
    for (uint32_t l = 0; l + 1u < knots; ++l) {              // (wave-uniform)
        const float t = __builtin_fminf(__builtin_fmaxf((zc - prof->k[l].z) * prof->k[l].inv, 0.0f), 1.0f);
        p[0] = __builtin_fmaf(prof->k[l].d[0], t, p[0]);
        p[1] = __builtin_fmaf(prof->k[l].d[1], t, p[1]);
        p[2] = __builtin_fmaf(prof->k[l].d[2], t, p[2]);
    }
    u[0] = u[0] + p[0]; u[1] = u[1] + p[1]; u[2] = u[2] + p[2];
}

// DepthEnsembleView with sheared_water for the water: begin (the member's table) and restore are inherited.
struct ShearedDepthView : DepthEnsembleView {
    const void* knot_table;
    uint32_t knots;
    __device__ __forceinline__ void view(uint32_t k, float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS]) const
    {
        float eta, u[3];
        sheared_water((SpectrumTablePtr)tab, waves, step0 + (int64_t)k, dt, s[0], s[1], s[2], HYDRO_FD_ARGS, (CurrentTablePtr)knot_table, knots, eta, u);
        float* m = parked();
        m[0] = s[2];
        s[2] = s[2] - eta;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            m[(1 + i) * 64] = s[7 + i];
            m[(4 + i) * 64] = pv[i];
            s[7 + i] = s[7 + i] - u[i];
            pv[i] = pv[i] - u[i];
        }
    }
};
__device__ __forceinline__ ShearedDepthView sheared_depth_view(HYDRO_SEA_PARAMS, HYDRO_ENS_PARAMS, HYDRO_FD_PARAMS, HYDRO_SHEAR_PARAMS)
{
    return ShearedDepthView{depth_ensemble_view(HYDRO_SEA_ARGS, HYDRO_ENS_ARGS, HYDRO_FD_ARGS), HYDRO_SHEAR_ARGS};
}

// The _fd kernel's arguments, then the knot table and its count.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_shear_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                   HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_SPREAD_PARAMS,
                                                                                                   HYDRO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS, HYDRO_ENS_PARAMS,
                                                                                                   HYDRO_FD_PARAMS, HYDRO_SHEAR_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   sheared_depth_view(HYDRO_SEA_ARGS, HYDRO_ENS_ARGS, HYDRO_FD_ARGS, HYDRO_SHEAR_ARGS),
                                                   optional_seabed_contact(HYDRO_OPT_BED_ARGS),
                                                   mooring_spread(HYDRO_SPREAD_ARGS), optional_extremes_track(HYDRO_EXT_ARGS),
                                                   OptionalPeakTetherNet{{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr}});
}

// The _fd_stat kernel's arguments, then the knot table and its count.
template <bool HALF, bool NT, bool IMPLICIT, bool KE, bool WARP>
__global__ void __launch_bounds__(kBlock) HYDRO_MULTI_OCC_ATTR step_fused_multi_shear_stat_tiled_kernel(HYDRO_BASE_PARAMS, HYDRO_REC_PARAMS, HYDRO_APP_PARAMS, HYDRO_CTL_PARAMS,
                                                                                                        HYDRO_SEA_PARAMS, HYDRO_OPT_BED_PARAMS, HYDRO_SPREAD_PARAMS,
                                                                                                        HYDRO_EXT_PARAMS, HYDRO_NET_PARAMS, HYDRO_PEAK_PARAMS, HYDRO_STAT_PARAMS,
                                                                                                        HYDRO_ENS_PARAMS, HYDRO_FD_PARAMS, HYDRO_SHEAR_PARAMS)
{
    fused_multi_body<HALF, NT, IMPLICIT, KE, WARP>(HYDRO_BASE_ARGS, optional_recorder(HYDRO_REC_ARGS), optional_pose_hold(HYDRO_APP_ARGS, HYDRO_CTL_ARGS),
                                                   sheared_depth_view(HYDRO_SEA_ARGS, HYDRO_ENS_ARGS, HYDRO_FD_ARGS, HYDRO_SHEAR_ARGS),
                                                   optional_seabed_contact(HYDRO_OPT_BED_ARGS),
                                                   mooring_spread(HYDRO_SPREAD_ARGS), statistics_track(HYDRO_EXT_ARGS, HYDRO_STAT_ARGS, steps),
                                                   OptionalPeakTetherNet{{{HYDRO_NET_ARGS, nullptr, 0u}, HYDRO_PEAK_ARGS, nullptr}});
}

// hydro_current_profile_sample: depth_sample_kernel calling sheared_water.
__global__ void __launch_bounds__(kBlock) shear_sample_kernel(const float* st, uint32_t st_stride, float* out, uint32_t out_stride, uint32_t n,
                                                              const void* sea_table, uint32_t sea_waves, int64_t step, double sea_dt, HYDRO_ENS_PARAMS, HYDRO_FD_PARAMS,
                                                              HYDRO_SHEAR_PARAMS)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const float* r = st + (size_t)tile * st_stride;
    float eta, u[3];
    sheared_water(ensemble_member((SpectrumTablePtr)sea_table, tile, tiles_per_sea), sea_waves, step, sea_dt, *at<float>(r, lane4, 0u), *at<float>(r, lane4, 256u),
                  *at<float>(r, lane4, 512u), HYDRO_FD_ARGS, (CurrentTablePtr)knot_table, knots, eta, u);
    const float o[HYDRO_SEA_FIELDS] = {eta, u[0], u[1], u[2]};
    store_record<HYDRO_SEA_FIELDS, false>(out + (size_t)tile * out_stride, lane4, o);
}

// --------------------------------------------------------------------------
// IRREGULAR and FINITE-DEPTH seas in the OPEN-LOOP steps (hydro_step_wrench_tiled_irr, hydro_step_wrench_aos_irr): the two
// open-loop sea kernels over again with spectrum_water or depth_water (DEPTH) for the water, against the table of the member
// the wave's tile steps through.  New kernels beside wrench_tiled_sea_kernel and wrench_aos_sea_kernel, which stay as they
// are; the host launches these only while a spectrum, an ensemble or a finite-depth sea is set.
//   time   : as in the _sea kernels, (step, sea_dt) = (1, time) or (0, time): spectrum_water and depth_water stay the only
//            implementations of the water, and the three *_sample kernels give the same bits
//   member : ensemble_member of the wave's tile; a lone spectrum is an ensemble of one, launched with a tiles_per_sea that no
//            tile index reaches (member 0 for every wave)
//   table  : stays in the constant address space: scalar loads in every trip of the component loops, nothing kept per component
//   prev   : the _sea kernels' rule - the TRUE velocity goes to the engine's record before the relative values are formed
// --------------------------------------------------------------------------
// (Depth: HYDRO_FD_PARAMS' one float with DEPTH, nothing without - the deep kernels take no depth argument)
template <bool DEPTH, typename... Depth>
__device__ __forceinline__ void irregular_relative(SpectrumTablePtr tab, uint32_t waves, int64_t step, double sea_dt,
                                                   float (&s)[HYDRO_STATE_FIELDS], float (&pv)[HYDRO_PREV_FIELDS], Depth... neg_depth)
{
    static_assert(sizeof...(Depth) == (DEPTH ? 1 : 0), "HYDRO_FD_PARAMS with DEPTH only");
    float eta, u[3];
    if constexpr (DEPTH) depth_water(tab, waves, step, sea_dt, s[0], s[1], s[2], neg_depth..., eta, u);
    else spectrum_water(tab, waves, step, sea_dt, s[0], s[1], s[2], eta, u);
    s[2] = s[2] - eta;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s[7 + i] = s[7 + i] - u[i];
        pv[i] = pv[i] - u[i];
    }
}

// wrench_tiled_sea_kernel's frame and first arguments (the same 16 preloaded dwords), then the sea's, the ensemble's and, with DEPTH, the depth (HYDRO_FD_PARAMS).
template <bool HALF, bool ENGINE_PREV, bool NT, bool WARP, bool DEPTH, typename... Depth>
__global__ void __launch_bounds__(kBlock) HYDRO_TILED_OCC_ATTR wrench_tiled_irr_kernel(const float* k_st, const float* k_pv, const float* k_prm, float* k_out, float* k_pv_out,
                                                             uint32_t st_stride, uint32_t pv_stride, uint32_t out_stride, uint32_t pvo_stride,
                                                             uint32_t n, int warp, double rho, double g, double inv_dt,
                                                             HYDRO_SEA_PARAMS, HYDRO_ENS_PARAMS, Depth... neg_depth)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u;
    const uint32_t first = tile * 64u;
    const uint32_t left = n - __builtin_amdgcn_readfirstlane(n < first ? n : first);       // (scalar, see wrench_tiled_kernel)
    if (lane >= left) return;
    const uint32_t lane4 = lane * 4u;
    float s[HYDRO_STATE_FIELDS], pv[HYDRO_PREV_FIELDS], d[3], c[7], mass, f6[HYDRO_WRENCH_FIELDS];
    load_tile_records<HALF, NT>(k_st + (size_t)tile * st_stride, k_pv + (size_t)tile * pv_stride, k_prm, tile, lane4, s, pv, d, c, mass);
    if constexpr (ENGINE_PREV) store_record<HYDRO_PREV_FIELDS, NT>(k_pv_out + (size_t)tile * pvo_stride, lane4, s + 7);
    const SpectrumTablePtr tab = ensemble_member((SpectrumTablePtr)sea_table, tile, HYDRO_ENS_ARGS);
    irregular_relative<DEPTH>(tab, sea_waves, step0, sea_dt, s, pv, HYDRO_FD_ARGS...);
    wrench_fields(body_wrench(s, pv, d, c, mass, rho, g, inv_dt, WARP), f6);
    store_record<HYDRO_WRENCH_FIELDS, NT>(k_out + (size_t)tile * out_stride, lane4, f6);
}

// wrench_aos_sea_kernel's frame and first arguments, then the sea's, the ensemble's and, with DEPTH, the depth (HYDRO_FD_PARAMS).
template <bool HALF, bool NT, bool WARP, bool DEPTH, typename... Depth>
__global__ void __launch_bounds__(kBlock) wrench_aos_irr_kernel(const float* k_pos, const float* k_quat, const float* k_vel, float* k_force, float* k_torque,
                                                               float* k_pv, const float* k_prm, int quat_xyzw, uint32_t n,      // 16 dwords: preloaded
                                                               int warp, double rho, double g, double inv_dt,
                                                               HYDRO_SEA_PARAMS, HYDRO_ENS_PARAMS, Depth... neg_depth)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const size_t first = (size_t)tile * 64u;
    const float* t_pos = k_pos + first * 3; const float* t_quat = k_quat + first * 4; const float* t_vel = k_vel + first * 6;
    float s[HYDRO_STATE_FIELDS], pv[HYDRO_PREV_FIELDS], d[3], c[7], mass;
    constexpr bool RNT = false;                              // (the simulator's rows: temporal, see wrench_aos_direct_kernel)
    const f3_a4 p = ld_f3_a4<RNT>(t_pos, lane * 12u);
    const f4_a16 q = ld_f4_a16<RNT>(t_quat, lane * 16u);
    const f4_a8 v0 = ld_f4_a8<RNT>(t_vel, lane * 24u);
    const f2_a8 v1 = ld_f2_a8<RNT>(t_vel, lane * 24u + 16u);
    s[0] = p.x; s[1] = p.y; s[2] = p.z;
    if (quat_xyzw) { s[3] = q.x; s[4] = q.y; s[5] = q.z; s[6] = q.w; }
    else           { s[3] = q.y; s[4] = q.z; s[5] = q.w; s[6] = q.x; }
    s[7] = v0.x; s[8] = v0.y; s[9] = v0.z; s[10] = v0.w; s[11] = v1.x; s[12] = v1.y;
    float* t_pv = k_pv + (size_t)tile * (HYDRO_PREV_FIELDS * HYDRO_TILE);
#pragma unroll
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) pv[f] = ldg<NT>(at<float>(t_pv, lane4, f * 256u));
    load_param_record<HALF, NT>(k_prm, tile, lane4, d, c, mass);
#pragma unroll
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) stg_aos<NT>(at<float>(t_pv, lane4, f * 256u), s[7 + f]);     // the TRUE velocity
    const SpectrumTablePtr tab = ensemble_member((SpectrumTablePtr)sea_table, tile, HYDRO_ENS_ARGS);
    irregular_relative<DEPTH>(tab, sea_waves, step0, sea_dt, s, pv, HYDRO_FD_ARGS...);
    const hydro::Wrench w = body_wrench(s, pv, d, c, mass, rho, g, inv_dt, WARP);
    f3_a4 fo, to;
    fo.x = w.fx; fo.y = w.fy; fo.z = w.fz; to.x = w.tx; to.y = w.ty; to.z = w.tz;
    st_f3_a4<NT>(k_force + first * 3, lane * 12u, fo);
    st_f3_a4<NT>(k_torque + first * 3, lane * 12u, to);
}

// hydro_statistics_reset: the empty record - sums +0.0, words 0 - for the live lanes.
__global__ void __launch_bounds__(kBlock) statistics_reset_kernel(void* stat, uint32_t stat_stride, uint32_t n)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    char* r = reinterpret_cast<char*>(reinterpret_cast<float*>(stat) + (size_t)tile * stat_stride);
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) *at<double>(r, lane4 * 2u, j * 512u) = 0.0;
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) *at<uint32_t>(r, lane4, kStatWordsAt + c * 256u) = 0u;
}

// hydro_tether_wrench: the tether's W per body for the tiled state `st` (+0 in all six fields for a body whose line adds
// nothing) and, if asked for, its tension T (+0 likewise).  The lanes >= n of the last tile leave first: the live ones
// exchange among themselves, in uniform control flow.
__global__ void __launch_bounds__(kBlock) tether_wrench_kernel(const float* st, uint32_t st_stride, const float* teth, uint32_t teth_stride,
                                                               float* out, uint32_t out_stride, float* tension, uint32_t tension_stride, uint32_t n)
{
    const uint32_t tile = wave_tile<kBlock>(blockIdx.x), lane = threadIdx.x & 63u, lane4 = lane * 4u;
    if (tile * 64u + lane >= n) return;
    const float* r = st + (size_t)tile * st_stride;
    float s[HYDRO_STATE_FIELDS], W[HYDRO_WRENCH_FIELDS], T = 0.0f;
#pragma unroll
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) s[f] = *at<float>(r, lane4, f * 256u);
    if (!tether_wrench(teth + (size_t)tile * teth_stride + lane, s, W, T)) {
#pragma unroll
        for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) W[f] = 0.0f;
        T = 0.0f;
    }
    store_record<HYDRO_WRENCH_FIELDS, false>(out + (size_t)tile * out_stride, lane4, W);
    if (tension) store_record<1, false>(tension + (size_t)tile * tension_stride, lane4, &T);    // (a kernel argument: wave-uniform)
}

// LaneSlots<SLOTS>::slots() is ONE __shared__ array per value of SLOTS: two policies of the same count that meet in one kernel
// (pose hold, sea view, mooring line and extremes all do, in step_fused_multi_ext_tiled_kernel) would park their values on top
// of each other without a message.  A new policy takes a count of its own (or LaneSlots grows a tag type).
constexpr bool lane_slot_counts_distinct(std::initializer_list<uint32_t> counts)
{
    for (auto a = counts.begin(); a != counts.end(); ++a)
        for (auto b = a + 1; b != counts.end(); ++b)
            if (*a == *b) return false;
    return true;
}
static_assert(lane_slot_counts_distinct({kCtlSlots, kSeaSlots, kMoorSlots, kExtSlots, kStatSlots}),
              "two LaneSlots policies of one kernel share a slot count, hence one LDS array");

}  // namespace

// ==========================================================================
// engine object + C ABI
// ==========================================================================
struct hydro_engine {
    int device = 0;
    int64_t capacity = 0;
    int64_t stride = 0;            // padded field stride of the engine-owned SoA buffers (floats)
    int64_t n_params = 0;          // bodies for which parameters have been set
    double rho = 1025.0, g = 9.81;
    int semantics = HYDRO_SEM_NUMBA;
    bool half_coeffs = false;
    // What the engine holds for every body: the tiled parameter record (44 B) and the tiled previous velocity (24 B).
    float* params_tiled = nullptr; // [tiles][11][64] f32 or [tiles][480] (fp16-coefficient record)
    float* prev_tiled = nullptr;   // [tiles][6][64]
    // Plain-SoA copies, made on the FIRST use of an entry point that takes plain field pointers (hydro_step_wrench,
    // _ext, hydro_step_components) and kept up to date from then on: a caller of the tiled / array-of-structs /
    // fused entries never pays their 82 B per body.
    float* params = nullptr;       // [11][stride] fp32
    __half* coeffs16 = nullptr;    // [7][stride]   (fp16-coefficient mode)
    float* prev = nullptr;         // [6][stride]
    bool soa_params_valid = false; // `params` / `coeffs16` reflect params_tiled
    double* ke_partials = nullptr; // [2][ke_stride]: one fp64 pair per block of 256 bodies
    uint32_t ke_stride = 0;
    // The reduction's ticket counters are zero between launches that finish.  ke_suspect: something went wrong on this
    // handle (a HIP call failed, or the caller says so: hydro_ke_rearm) - the next kinetic-energy launch zeroes them first.
    // ke_last_stream: where the previous such launch went; a launch on ANOTHER stream is ordered behind it (ke_event).
    bool ke_suspect = false;
    bool ke_launched = false;
    hipStream_t ke_last_stream = nullptr;
    hipEvent_t ke_event = nullptr;
    // The trajectory recorder's watch list (hydro_set_watch): per tile of the capacity, the mask of watched lanes and the
    // log column of the first of them (hydro_watch.h); allocated by the first hydro_set_watch, kept until hydro_destroy.
    uint64_t* watch_mask = nullptr;  // [tiles of capacity]
    uint32_t* watch_first = nullptr; // [tiles of capacity]
    int64_t watch_count = 0;         // 0: no watch list
    int64_t watch_last = -1;         // the largest watched body (a recording launch needs it below its n)
    // The sea state (hydro_set_sea): the device table the sea kernels read (SeaTable), allocated by the first hydro_set_sea,
    // kept until hydro_destroy.  sea_waves < 0: no sea.
    void* sea_table = nullptr;
    int sea_waves = -1;
    // The sea spectrum (hydro_set_sea_spectrum): the device table the _irr kernels read (SpectrumTable), allocated by the first
    // hydro_set_sea_spectrum, kept until hydro_destroy.  spectrum_waves < 0: no spectrum.  Never set together with a sea.
    void* spectrum_table = nullptr;
    int spectrum_waves = -1;
    // The sea ensemble (hydro_set_sea_ensemble): `ensemble_count` SpectrumTables one behind the other, the device table allocated
    // for `ensemble_capacity` members by the first call that needs as many, kept until hydro_destroy.  ensemble_waves < 0: no
    // ensemble.  Never set together with a sea or a spectrum.
    void* ensemble_table = nullptr;
    int64_t ensemble_capacity = 0, ensemble_count = 0, ensemble_tiles_per_sea = 0;
    int ensemble_waves = -1;
    // The finite-depth sea (hydro_set_sea_finite_depth): the ensemble's table over again, of its own - the records hold the
    // constants scaled by 1 / (1 - q_j) and gl_j in `pad` - with -h rounded once to fp32, a kernel argument.  fd_waves < 0: no
    // finite-depth sea.  Never set together with a sea, a spectrum or an ensemble.
    void* fd_table = nullptr;
    int64_t fd_capacity = 0, fd_count = 0, fd_tiles_per_sea = 0;
    int fd_waves = -1;
    float fd_neg_depth = 0.0f;
    // The current profile (hydro_set_current_profile): the device table the _shear kernels read (CurrentTable), allocated by the
    // first hydro_set_current_profile, kept until hydro_destroy.  shear_knots == 0: no profile.  Independent of the kind of sea.
    void* shear_table = nullptr;
    int shear_knots = 0;
    // The seabed (hydro_set_seabed): the plane and the five contact constants, already rounded to fp32 - kernel arguments.
    Seabed bed = {};
    bool has_bed = false;
    hipStream_t stream = nullptr;
    int vec = 0;                   // bodies per lane, 0 = default (1)
    int block = 0;                 // threads per block, 0 = by size
    int nt = -1;                   // non-temporal accesses: -1 = by size, 0 = off, 1 = on
    int waves = -1;                // resident waves per SIMD of the tiled wrench kernel: -1 = by size, 0 = no cap
    // the engine-owned previous velocity may exist in both layouts; which copy is current (a plain-SoA copy that has
    // not been allocated yet counts as stale):
    enum PrevCopy { kPrevBoth, kPrevSoa, kPrevTiled } prev_current = kPrevTiled;
    char err[512] = {0};
};

namespace {

int fail(hydro_engine* h, int code, const char* what, hipError_t e = hipSuccess)
{
    if (h) {
        if (e != hipSuccess) {
            snprintf(h->err, sizeof h->err, "%s: %s", what, hipGetErrorString(e));
            h->ke_suspect = true;             // a launch of this handle may not have run to its end: re-arm the reduction
        }
        else snprintf(h->err, sizeof h->err, "%s", what);
    }
    return code;
}

#define HYDRO_HIP(h, call, code)                                   \
    do {                                                           \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess) return fail((h), (code), #call, e_); \
    } while (0)

// Make the engine's device current only when it is not already (hipGetDevice is a thread-local read; a step
// call from a single-GPU host then skips the hipSetDevice round trip).
inline hipError_t use_device(int device)
{
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device) return hipSuccess;
    return hipSetDevice(device);
}

inline int grid_for(int64_t n, int per_block) { return (int)((n + per_block - 1) / per_block); }

bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

int check_common(hydro_engine* h, int64_t n)
{
    if (!h) return HYDRO_E_ARG;
    if (n < 0 || n > h->capacity) return fail(h, HYDRO_E_ARG, "n out of range (0 <= n <= capacity)");
    if (n > h->n_params) return fail(h, HYDRO_E_STATE, "parameters not set for n bodies (call hydro_set_params_* first)");
    return HYDRO_OK;
}

template <typename Args>
void fill_params(hydro_engine* h, Args& a)
{
    for (int f = 0; f < 3; ++f) a.dims[f] = h->params + f * h->stride;
    for (int f = 0; f < 7; ++f)
        a.coef[f] = h->half_coeffs ? static_cast<const void*>(h->coeffs16 + f * h->stride)
                                   : static_cast<const void*>(h->params + (3 + f) * h->stride);
}

// tiled parameter record: floats per tile and the field that holds the mass
inline uint32_t prm_tile_floats(const hydro_engine* h) { return h->half_coeffs ? kPrmTileF16 : kPrmTileF32; }
inline uint32_t prm_mass_field(const hydro_engine* h) { return h->half_coeffs ? 3u : 10u; }

// The plain-SoA copies of the parameters (for the entry points that take plain field pointers).  They are ALLOCATED on
// the first use of such an entry, or by hydro_reserve_soa; once they exist every hydro_set_params_* refreshes them in
// place (it synchronises anyway), so the step path itself never allocates or synchronises again - which is what makes
// a plain-SoA step capturable after hydro_reserve_soa, in any order with hydro_set_params_*.
int refresh_soa_params(hydro_engine* h)
{
    if (h->n_params > 0) {
        hipLaunchKernelGGL(params_from_tiled_kernel, dim3(grid_for(h->n_params, kBlock)), dim3(kBlock), 0, h->stream,
                           h->params_tiled, h->half_coeffs ? 1 : 0, h->params, h->stride, h->coeffs16, (uint32_t)h->n_params);
        HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
        HYDRO_HIP(h, hipStreamSynchronize(h->stream), HYDRO_E_LAUNCH);      // later calls may come on other streams
    }
    h->soa_params_valid = true;
    return HYDRO_OK;
}

int ensure_soa_params(hydro_engine* h)
{
    const size_t fbytes = sizeof(float) * (size_t)h->stride;
    if (!h->params && hipMalloc(&h->params, fbytes * HYDRO_PARAM_FIELDS) != hipSuccess)
        return fail(h, HYDRO_E_ALLOC, "plain-SoA parameter copy: allocation failed (first use of a plain-SoA entry point allocates; not inside a graph capture)");
    // (the fp16 copy is allocated with the fp32 one, whatever the current mode: hydro_set_params_f16 may come later)
    if (!h->coeffs16 && hipMalloc(&h->coeffs16, sizeof(__half) * (size_t)h->stride * 7) != hipSuccess) {
        // both or neither: hydro_set_params_* refreshes the copies whenever `params` exists, and writes both
        (void)hipFree(h->params);
        h->params = nullptr; h->coeffs16 = nullptr; h->soa_params_valid = false;
        return fail(h, HYDRO_E_ALLOC, "plain-SoA fp16 coefficient copy: allocation failed");
    }
    return h->soa_params_valid ? HYDRO_OK : refresh_soa_params(h);
}

// the six fields of the engine's plain-SoA previous velocity
struct PrevRows { float* f[HYDRO_PREV_FIELDS]; };
inline PrevRows prev_rows(const hydro_engine* h)
{
    PrevRows r;
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) r.f[f] = h->prev + f * h->stride;
    return r;
}

int ensure_soa_prev(hydro_engine* h)
{
    if (h->prev) return HYDRO_OK;
    const size_t bytes = sizeof(float) * (size_t)h->stride * HYDRO_PREV_FIELDS;
    if (hipMalloc(&h->prev, bytes) != hipSuccess)
        return fail(h, HYDRO_E_ALLOC, "plain-SoA previous-velocity copy: allocation failed (first use of hydro_step_wrench allocates; not inside a graph capture)");
    HYDRO_HIP(h, hipMemsetAsync(h->prev, 0, bytes, h->stream), HYDRO_E_LAUNCH);
    HYDRO_HIP(h, hipStreamSynchronize(h->stream), HYDRO_E_LAUNCH);
    if (h->prev_current == hydro_engine::kPrevBoth) h->prev_current = hydro_engine::kPrevTiled;   // the new copy is stale
    return HYDRO_OK;
}

// Launch geometry, measured on MI355X (interleaved A/B of whole libraries, scripts/ab_variants.py):
//   * non-temporal accesses: +5..9 % once the scene is larger than the caches; small scenes keep
//     temporal accesses so that a few-MB working set stays L2 / Infinity-Cache resident between steps;
//   * block size: with the fp64 body 128- and 256-thread blocks of the tiled kernel measure the same at 1M bodies
//     (+-0.1 us) and 256 is 1-2 us faster at 4M: the tiled kernel always launches 256.  (Round 1's fp32 body gained
//     8..12 % from 128-thread blocks around 1M; the plain-SoA kernel keeps that rule below 2M bodies.)
constexpr int64_t kNtMinBodies = 131072;
// The fused step is the closed-loop kernel: ONE scene stepping on itself (state ping-pong + parameters,
// ~150 B of working set per body).  Between ~0.45M and ~2.6M bodies that set fits, or mostly fits, the 256 MiB
// Infinity Cache, and leaving the accesses temporal lets step k+1 find step k's output there: measured
// (scripts/diag_mall.py, hipGraph x64) 16.5 vs 19.2 us at 0.5M, 28.9 vs 33.5 us at 1M, 41.0 vs 45.6 us at 1.5M,
// 55.1 vs 58.5 us at 2M; below (L2-sized sets) and above (thrashing) non-temporal wins by 4-12 %.
constexpr int64_t kFusedTemporalMin = 458752, kFusedTemporalMax = 2621440;
constexpr int64_t kBigBlockMinBodies = 2097152;

// streaming (non-temporal) accesses: by the size of the launch unless hydro_set_tuning says otherwise
inline bool streaming(const hydro_engine* h, int64_t n) { return h->nt < 0 ? n >= kNtMinBodies : h->nt != 0; }
inline bool streaming_fused(const hydro_engine* h, int64_t n)
{
    return h->nt < 0 ? n >= kNtMinBodies && !(n >= kFusedTemporalMin && n <= kFusedTemporalMax) : h->nt != 0;
}
inline bool is_warp(const hydro_engine* h) { return h->semantics == HYDRO_SEM_WARP; }

// Which instantiation of a kernel a launch takes: N run-time flags become N compile-time ones.  f is called once, with a
// std::true_type or std::false_type per flag in the order of the flags; a generic lambda uses them as template arguments.
template <typename F> void dispatch_flags(F&& f) { f(); }
template <typename F, typename... Rest> void dispatch_flags(F&& f, bool b, Rest... rest)
{
    if (b) dispatch_flags([&](auto... done) { f(std::true_type{}, done...); }, rest...);
    else dispatch_flags([&](auto... done) { f(std::false_type{}, done...); }, rest...);
}

template <int VEC, bool WRITE_PREV>
void launch_soa_n(hydro_engine* h, const SoaArgs& a, hipStream_t s, int64_t n_total)
{
    const int block = h->block ? h->block : (n_total >= kBigBlockMinBodies ? 256 : 128);
    dispatch_flags([&](auto BIG, auto HALF, auto NT, auto WARP) {
        constexpr int BLOCK = BIG ? 256 : 128;
        hipLaunchKernelGGL((wrench_soa_kernel<BLOCK, VEC, HALF, WRITE_PREV, NT, WARP>), dim3(grid_for(a.n, BLOCK * VEC)), dim3(BLOCK), 0, s, a);
    }, block == 256, h->half_coeffs, streaming(h, n_total), is_warp(h));
}

// args shifted by `off` bodies (for the ragged remainder of a vector launch)
SoaArgs shifted(const SoaArgs& a, int64_t off, int64_t n, bool half)
{
    SoaArgs b = a;
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) b.st[f] = a.st[f] + off;
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) { b.pv[f] = a.pv[f] + off; b.pv_out[f] = a.pv_out[f] ? a.pv_out[f] + off : nullptr; }
    for (int f = 0; f < 3; ++f) b.dims[f] = a.dims[f] + off;
    for (int f = 0; f < 7; ++f)
        b.coef[f] = half ? static_cast<const void*>(static_cast<const __half*>(a.coef[f]) + off)
                         : static_cast<const void*>(static_cast<const float*>(a.coef[f]) + off);
    b.mass = a.mass + off;
    for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) b.out[f] = a.out[f] + off;
    b.n = n;
    return b;
}

template <int VEC, bool WRITE_PREV>
void launch_soa(hydro_engine* h, const SoaArgs& a, hipStream_t s)
{
    const int64_t n_vec = a.n / VEC * VEC;
    if (n_vec > 0) {
        SoaArgs b = a;
        b.n = n_vec;
        launch_soa_n<VEC, WRITE_PREV>(h, b, s, a.n);
    }
    if constexpr (VEC > 1) {
        if (a.n > n_vec) launch_soa_n<1, WRITE_PREV>(h, shifted(a, n_vec, a.n - n_vec, h->half_coeffs), s, a.n);
    }
}

// The argument checks of a plain-SoA step, in the order the errors are reported.  with_prev = false leaves the previous
// velocity out: hydro_step_wrench must pass the others before it touches (allocates, repacks) its own copy of it.
int check_soa_step(hydro_engine* h, int64_t n, const float* const state[], const float* const prev[], bool with_prev,
                   double dt, float* const wrench[])
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (!state || !wrench || (with_prev && !prev)) return fail(h, HYDRO_E_ARG, "null pointer table");
    if (!(dt > 0.0)) return fail(h, HYDRO_E_ARG, "dt must be > 0");
    if (n == 0) return HYDRO_OK;
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) if (!state[f]) return fail(h, HYDRO_E_ARG, "null state field");
    for (int f = 0; with_prev && f < HYDRO_PREV_FIELDS; ++f) if (!prev[f]) return fail(h, HYDRO_E_ARG, "null previous-velocity field");
    for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) if (!wrench[f]) return fail(h, HYDRO_E_ARG, "null wrench field");
    return HYDRO_OK;
}

template <bool WRITE_PREV>
int step_soa(hydro_engine* h, int64_t n, const float* const state[], const float* const prev[], float* const prev_out[],
             double dt, float* const wrench[], void* stream)
{
    int rc = check_soa_step(h, n, state, prev, true, dt, wrench);
    if (rc || n == 0) return rc;
    SoaArgs a;
    int vec = h->vec ? h->vec : 1;          // bodies per lane: what every field pointer's alignment allows
    const auto fit = [&vec](const void* p) { while (vec > 1 && !aligned_to(p, sizeof(float) * vec)) vec >>= 1; };
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) { a.st[f] = state[f]; fit(state[f]); }
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) { a.pv[f] = prev[f]; a.pv_out[f] = prev_out ? prev_out[f] : nullptr; fit(prev[f]); }
    for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) { a.out[f] = wrench[f]; fit(wrench[f]); }
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = ensure_soa_params(h))) return rc;                    // plain-SoA parameter copies: made on first use
    fill_params(h, a);
    a.mass = h->params + 10 * h->stride;
    a.rho = h->rho; a.g = h->g; a.warp = h->semantics;
    a.inv_dt = 1.0 / dt;
    a.n = n;
    if (vec >= 2) launch_soa<2, WRITE_PREV>(h, a, s);
    else launch_soa<1, WRITE_PREV>(h, a, s);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

// A temporary device copy of `nfields` host arrays of n floats ([nfields][n]); the caller frees it.
int stage_host_fields(hydro_engine* h, const float* const src[], int nfields, int64_t n, float** staged)
{
    *staged = nullptr;
    if (hipMalloc(staged, sizeof(float) * (size_t)n * nfields) != hipSuccess) return fail(h, HYDRO_E_ALLOC, "staging buffer: allocation failed");
    for (int f = 0; f < nfields; ++f) {
        hipError_t e = hipMemcpyAsync(*staged + (size_t)f * n, src[f], sizeof(float) * n, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) { (void)hipFree(*staged); *staged = nullptr; return fail(h, HYDRO_E_LAUNCH, "hipMemcpyAsync (host -> device)", e); }
    }
    return HYDRO_OK;
}

int set_params(hydro_engine* h, int64_t n, const float* const params[], int on_device, bool half)
{
    if (!h) return HYDRO_E_ARG;
    if (!params) return fail(h, HYDRO_E_ARG, "null pointer table");
    if (n < 0 || n > h->capacity) return fail(h, HYDRO_E_ARG, "n out of range (0 <= n <= capacity)");
    for (int f = 0; f < HYDRO_PARAM_FIELDS; ++f) if (!params[f]) return fail(h, HYDRO_E_ARG, "null field pointer");
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (n > 0) {
        // straight from the caller's arrays into the tiled records (host arrays go through a temporary device copy)
        ParamPtrs src;
        float* staged = nullptr;
        if (on_device) {
            for (int f = 0; f < HYDRO_PARAM_FIELDS; ++f) src.f[f] = params[f];
        } else {
            int rc = stage_host_fields(h, params, HYDRO_PARAM_FIELDS, n, &staged);
            if (rc) return rc;
            for (int f = 0; f < HYDRO_PARAM_FIELDS; ++f) src.f[f] = staged + (size_t)f * n;
        }
        if (half) {
            // before anything is written: no finite coefficient may become +-Inf in the half record (the previous record stays)
            unsigned long long* flag = nullptr;
            unsigned long long first_bad = ~0ull;
            if (hipMalloc(&flag, sizeof first_bad) != hipSuccess) {
                if (staged) (void)hipFree(staged);
                return fail(h, HYDRO_E_ALLOC, "hydro_set_params_f16: allocation of the range check's flag failed");
            }
            hipError_t e = hipMemsetAsync(flag, 0xff, sizeof first_bad, h->stream);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(params_f16_range_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, h->stream, src, flag, (uint32_t)n);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(&first_bad, flag, sizeof first_bad, hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            (void)hipFree(flag);
            if (e != hipSuccess || first_bad != ~0ull) {
                if (staged) (void)hipFree(staged);
                if (e != hipSuccess) return fail(h, HYDRO_E_LAUNCH, "params_f16_range_kernel", e);
                static const char* const names[7] = {"cd_lin", "cd_ang", "damp_lin", "damp_ang", "lift", "am_lin", "am_ang"};
                char msg[256];
                snprintf(msg, sizeof msg, "hydro_set_params_f16: %s of body %llu is finite but at least 65520 in magnitude, which half "
                         "precision stores as Inf; nothing was written, the previous record stays: use hydro_set_params_f32",
                         names[first_bad & 7u], first_bad >> 3);
                return fail(h, HYDRO_E_ARG, msg);
            }
        }
        const uint32_t n_pad = (uint32_t)((n + 63) / 64 * 64);
        hipLaunchKernelGGL(params_to_tiled_kernel, dim3(grid_for(n_pad, kBlock)), dim3(kBlock), 0, h->stream,
                           src, h->params_tiled, half ? 1 : 0, n_pad, (uint32_t)n);
        hipError_t e = hipGetLastError();
        // the source arrays may be pageable host memory, or device memory that the caller frees right away
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (staged) (void)hipFree(staged);
        if (e != hipSuccess) return fail(h, HYDRO_E_LAUNCH, "params_to_tiled_kernel", e);
    }
    h->half_coeffs = half;
    h->n_params = n;
    h->soa_params_valid = false;
    if (h->params) return refresh_soa_params(h); // the plain-SoA copies exist (an entry point asked for them, or hydro_reserve_soa): keep them current
    return HYDRO_OK;
}

int repack(hydro_engine* h, float* const soa[], int fields, float* tiled, int64_t tile_stride, int64_t n, bool to_tiled, hipStream_t s)
{
    if (fields > 24) return fail(h, HYDRO_E_ARG, "too many fields");
    RepackArgs a;
    for (int f = 0; f < fields; ++f) a.soa[f] = soa[f];
    a.tiled = tiled; a.tile_stride = (uint32_t)tile_stride; a.fields = fields; a.to_tiled = to_tiled ? 1 : 0; a.n = (uint32_t)n;
    hipLaunchKernelGGL(repack_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, a);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int check_tiled(hydro_engine* h, int64_t n, const void* p, int64_t stride, int fields, const char* what)
{
    if (!p) return fail(h, HYDRO_E_ARG, what);
    if (stride < (int64_t)fields * HYDRO_TILE || stride % 4 != 0 || stride >= (1 << 24))
        return fail(h, HYDRO_E_ARG, "tile stride too small, too large (>= 2^24) or not a multiple of 4 floats");
    if (!aligned_to(p, 16)) return fail(h, HYDRO_E_ARG, "tiled buffers must be 16-byte aligned");
    // 32-bit byte offsets inside the kernels
    const int64_t tiles = (n + HYDRO_TILE - 1) / HYDRO_TILE;
    if (tiles * stride * 4 >= ((int64_t)1 << 32)) return fail(h, HYDRO_E_ARG, "tiled buffer exceeds 4 GiB: split the scene");
    return HYDRO_OK;
}

// the kinetic energy of no bodies (the kernels that sample it are not launched for n == 0)
int ke_of_nothing(hydro_engine* h, double* out_dev, hipStream_t s)
{
    HYDRO_HIP(h, hipMemsetAsync(out_dev, 0, 2 * sizeof(double), s), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

inline uint32_t* ke_counters(hydro_engine* h)
{
    return reinterpret_cast<uint32_t*>(h->ke_partials + 2 * (size_t)h->ke_stride + 2 * kKeClasses);
}
constexpr size_t kKeCounterBytes = (1 + kKeClasses) * 256;

// Before every launch that carries the kinetic-energy reduction (stand-alone or inside a step kernel), on its stream:
//   * a launch on a stream OTHER than the previous one's is ordered behind it - the scratch and the counters are the
//     engine's, two reductions in flight at once would draw each other's tickets.  Costs nothing while the caller stays on
//     one stream (a pointer compare).  Not done while either stream is being captured (an event from outside a capture
//     cannot be waited for inside one): a captured launch on a second stream stays the caller's business, as documented;
//   * then the ticket counters are zeroed if anything went wrong on this handle since the last one (ke_suspect) - after
//     the wait above, and never inside a capture.
int ke_prepare(hydro_engine* h, hipStream_t s)
{
    hipStreamCaptureStatus c_new = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &c_new) != hipSuccess || c_new != hipStreamCaptureStatusNone;
    // (1) order this stream behind the previous launch's FIRST: the memset below must not zero counters under a
    //     reduction that is still running on the other stream
    if (h->ke_launched && s != h->ke_last_stream && !capturing) {
        hipStreamCaptureStatus c_old = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(h->ke_last_stream, &c_old) == hipSuccess && c_old == hipStreamCaptureStatusNone) {
            if (!h->ke_event && hipEventCreateWithFlags(&h->ke_event, hipEventDisableTiming) != hipSuccess) h->ke_event = nullptr;
            // (the previous stream may be gone: a failed record means there is nothing left to wait for - its error, and only
            // its error, is dropped here; an error the caller's own code left pending is not this function's to swallow)
            if (h->ke_event) {
                if (hipEventRecord(h->ke_event, h->ke_last_stream) == hipSuccess)
                    HYDRO_HIP(h, hipStreamWaitEvent(s, h->ke_event, 0), HYDRO_E_LAUNCH);
                else
                    (void)hipGetLastError();   // the record's own error only (the launch checks that follow must not trip over it)
            }
        }
    }
    // (2) re-arm after a fault seen on this handle.  Not while `s` is being captured: a memset recorded into a graph runs
    //     at every replay, not now, and would leave an eager launch before the first replay un-rearmed - the flag stays
    //     set and the next launch outside a capture does it (hydro_ke_rearm does it on request).
    if (h->ke_suspect && !capturing) {
        HYDRO_HIP(h, hipMemsetAsync(ke_counters(h), 0, kKeCounterBytes, s), HYDRO_E_LAUNCH);
        h->ke_suspect = false;
    }
    h->ke_last_stream = s;
    h->ke_launched = true;
    return HYDRO_OK;
}

// Bring the copy of the engine-owned previous velocity that `want` names up to date (a repack
// kernel on the caller's stream when the other layout was written last), then mark it as the one
// that is about to be written.  The plain-SoA copy is allocated on its first use.
int prev_acquire(hydro_engine* h, hydro_engine::PrevCopy want, int64_t n, hipStream_t s)
{
    if (want == hydro_engine::kPrevSoa) {
        int rc = ensure_soa_prev(h);
        if (rc) return rc;
    }
    if (h->prev_current != hydro_engine::kPrevBoth && h->prev_current != want && n > 0) {
        const int64_t m = h->n_params;            // every body that may have been stepped
        int rc = repack(h, prev_rows(h).f, HYDRO_PREV_FIELDS, h->prev_tiled, HYDRO_PREV_FIELDS * HYDRO_TILE, m > n ? m : n,
                        want == hydro_engine::kPrevTiled, s);
        if (rc) return rc;
    }
    h->prev_current = want;
    return HYDRO_OK;
}

}  // namespace

extern "C" {

int hydro_version(void) { return HYDRO_VERSION; }

const char* hydro_status_string(int status)
{
    switch (status) {
        case HYDRO_OK: return "HYDRO_OK";
        case HYDRO_E_ARG: return "HYDRO_E_ARG";
        case HYDRO_E_ALLOC: return "HYDRO_E_ALLOC";
        case HYDRO_E_LAUNCH: return "HYDRO_E_LAUNCH";
        case HYDRO_E_DEVICE: return "HYDRO_E_DEVICE";
        case HYDRO_E_STATE: return "HYDRO_E_STATE";
        default: return "HYDRO_E_UNKNOWN";
    }
}

int hydro_device_count(int* count)
{
    if (!count) return HYDRO_E_ARG;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) { *count = 0; return HYDRO_E_DEVICE; }
    *count = c;
    return HYDRO_OK;
}

int hydro_create(int device, int64_t capacity, hydro_t** out)
{
    if (!out || capacity <= 0 || capacity > ((int64_t)1 << 30)) return HYDRO_E_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return HYDRO_E_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return HYDRO_E_DEVICE;
    hydro_engine* h = new (std::nothrow) hydro_engine();
    if (!h) return HYDRO_E_ALLOC;
    h->device = device;
    h->capacity = capacity;
    h->stride = (capacity + 1023) / 1024 * 1024;          // 4 KiB-aligned fields; a whole number of tiles
    h->ke_stride = (uint32_t)((capacity + kBlock - 1) / kBlock);
    const size_t fbytes = sizeof(float) * (size_t)h->stride;
    // 68 B per body: tiled parameters + tiled previous velocity (+ 1/16 B of reduction scratch).  The plain-SoA
    // copies (82 B per body more) come with the first call of an entry point that needs them.
    bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipMalloc(&h->params_tiled, fbytes * HYDRO_PARAM_FIELDS) == hipSuccess;
    ok = ok && hipMalloc(&h->prev_tiled, fbytes * HYDRO_PREV_FIELDS) == hipSuccess;
    ok = ok && hipMemsetAsync(h->prev_tiled, 0, fbytes * HYDRO_PREV_FIELDS, h->stream) == hipSuccess;
    // [2][ke_stride] partials + class sums and ticket counters of the reduction (zero between launches, see ke_block_reduce)
    const size_t ke_bytes = sizeof(double) * 2 * (size_t)h->ke_stride + kKeScratchTailBytes;
    ok = ok && hipMalloc(&h->ke_partials, ke_bytes) == hipSuccess;
    ok = ok && hipMemsetAsync(h->ke_partials, 0, ke_bytes, h->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(h->stream) == hipSuccess;
    if (!ok) { hydro_destroy(h); return HYDRO_E_ALLOC; }
    *out = h;
    return HYDRO_OK;
}

int hydro_destroy(hydro_t* h)
{
    if (!h) return HYDRO_E_ARG;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    if (h->params) (void)hipFree(h->params);
    if (h->coeffs16) (void)hipFree(h->coeffs16);
    if (h->prev) (void)hipFree(h->prev);
    if (h->params_tiled) (void)hipFree(h->params_tiled);
    if (h->prev_tiled) (void)hipFree(h->prev_tiled);
    if (h->ke_partials) (void)hipFree(h->ke_partials);
    if (h->ke_event) (void)hipEventDestroy(h->ke_event);
    if (h->watch_mask) (void)hipFree(h->watch_mask);
    if (h->watch_first) (void)hipFree(h->watch_first);
    if (h->sea_table) (void)hipFree(h->sea_table);
    if (h->spectrum_table) (void)hipFree(h->spectrum_table);
    if (h->ensemble_table) (void)hipFree(h->ensemble_table);
    if (h->fd_table) (void)hipFree(h->fd_table);
    if (h->shear_table) (void)hipFree(h->shear_table);
    delete h;
    return HYDRO_OK;
}

int hydro_reserve_soa(hydro_t* h)
{
    if (!h) return HYDRO_E_ARG;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    int rc = ensure_soa_params(h);
    if (rc) return rc;
    if ((rc = ensure_soa_prev(h))) return rc;
    if (h->prev_current == hydro_engine::kPrevTiled && h->n_params > 0) {      // bring the plain copy up to date
        if ((rc = repack(h, prev_rows(h).f, HYDRO_PREV_FIELDS, h->prev_tiled, HYDRO_PREV_FIELDS * HYDRO_TILE, h->n_params, false, h->stream))) return rc;
        HYDRO_HIP(h, hipStreamSynchronize(h->stream), HYDRO_E_LAUNCH);
        h->prev_current = hydro_engine::kPrevBoth;
    }
    return HYDRO_OK;
}

const char* hydro_last_error(const hydro_t* h) { return h ? h->err : "null handle"; }

int64_t hydro_capacity(const hydro_t* h) { return h ? h->capacity : 0; }

int hydro_set_scene(hydro_t* h, double water_density, double gravity)
{
    if (!h) return HYDRO_E_ARG;
    if (!(water_density >= 0.0) || !(gravity == gravity)) return fail(h, HYDRO_E_ARG, "bad scene scalars");
    h->rho = water_density;
    h->g = gravity;
    return HYDRO_OK;
}

int hydro_set_params_f32(hydro_t* h, int64_t n, const float* const params[HYDRO_PARAM_FIELDS], int on_device)
{
    return set_params(h, n, params, on_device, false);
}

int hydro_set_params_f16(hydro_t* h, int64_t n, const float* const params[HYDRO_PARAM_FIELDS], int on_device)
{
    return set_params(h, n, params, on_device, true);
}

int hydro_reset_prev_velocity(hydro_t* h)
{
    if (!h) return HYDRO_E_ARG;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (h->prev) HYDRO_HIP(h, hipMemsetAsync(h->prev, 0, sizeof(float) * (size_t)h->stride * HYDRO_PREV_FIELDS, h->stream), HYDRO_E_LAUNCH);
    HYDRO_HIP(h, hipMemsetAsync(h->prev_tiled, 0, sizeof(float) * (size_t)h->stride * HYDRO_PREV_FIELDS, h->stream), HYDRO_E_LAUNCH);
    HYDRO_HIP(h, hipStreamSynchronize(h->stream), HYDRO_E_LAUNCH);
    h->prev_current = h->prev ? hydro_engine::kPrevBoth : hydro_engine::kPrevTiled;
    return HYDRO_OK;
}

int hydro_get_prev_velocity(hydro_t* h, int64_t n, float* const prev[HYDRO_PREV_FIELDS], int on_device)
{
    if (!h) return HYDRO_E_ARG;
    if (!prev || n < 0 || n > h->capacity) return fail(h, HYDRO_E_ARG, "bad arguments");
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) if (!prev[f]) return fail(h, HYDRO_E_ARG, "null field pointer");
    if (n == 0) return HYDRO_OK;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (h->prev_current == hydro_engine::kPrevSoa) {              // last written by a plain-SoA step: that copy is the current one
        for (int f = 0; f < HYDRO_PREV_FIELDS; ++f)
            HYDRO_HIP(h, hipMemcpyAsync(prev[f], h->prev + f * h->stride, sizeof(float) * n,
                                        on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream), HYDRO_E_LAUNCH);
        HYDRO_HIP(h, hipStreamSynchronize(h->stream), HYDRO_E_LAUNCH);
        return HYDRO_OK;
    }
    // from the tiled records: straight into device arrays, through a temporary device copy into host arrays
    float* rows[HYDRO_PREV_FIELDS];
    float* staged = nullptr;
    if (on_device) {
        for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) rows[f] = prev[f];
    } else {
        if (hipMalloc(&staged, sizeof(float) * (size_t)n * HYDRO_PREV_FIELDS) != hipSuccess) return fail(h, HYDRO_E_ALLOC, "staging buffer: allocation failed");
        for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) rows[f] = staged + (size_t)f * n;
    }
    int rc = repack(h, rows, HYDRO_PREV_FIELDS, h->prev_tiled, HYDRO_PREV_FIELDS * HYDRO_TILE, n, false, h->stream);
    hipError_t e = hipSuccess;
    if (!rc && staged)
        for (int f = 0; f < HYDRO_PREV_FIELDS && e == hipSuccess; ++f)
            e = hipMemcpyAsync(prev[f], rows[f], sizeof(float) * n, hipMemcpyDeviceToHost, h->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (staged) (void)hipFree(staged);
    if (rc) return rc;
    if (e != hipSuccess) return fail(h, HYDRO_E_LAUNCH, "hydro_get_prev_velocity", e);
    return HYDRO_OK;
}

int hydro_set_prev_velocity(hydro_t* h, int64_t n, const float* const prev[HYDRO_PREV_FIELDS], int on_device)
{
    if (!h) return HYDRO_E_ARG;
    if (!prev || n < 0 || n > h->capacity) return fail(h, HYDRO_E_ARG, "bad arguments");
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) if (!prev[f]) return fail(h, HYDRO_E_ARG, "null field pointer");
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (n > 0) {
        // if a plain-SoA step ran last, the bodies beyond n keep what it left: bring the tiled records up to date first
        int rc = prev_acquire(h, hydro_engine::kPrevTiled, h->n_params, h->stream);
        if (rc) return rc;
        float* rows[HYDRO_PREV_FIELDS];
        float* staged = nullptr;
        if (on_device) {
            for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) rows[f] = const_cast<float*>(prev[f]);     // read only (to_tiled)
        } else {
            if ((rc = stage_host_fields(h, prev, HYDRO_PREV_FIELDS, n, &staged))) return rc;
            for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) rows[f] = staged + (size_t)f * n;
        }
        rc = repack(h, rows, HYDRO_PREV_FIELDS, h->prev_tiled, HYDRO_PREV_FIELDS * HYDRO_TILE, n, true, h->stream);
        const hipError_t e = hipStreamSynchronize(h->stream);
        if (staged) (void)hipFree(staged);
        if (rc) return rc;
        if (e != hipSuccess) return fail(h, HYDRO_E_LAUNCH, "hydro_set_prev_velocity", e);
    }
    h->prev_current = hydro_engine::kPrevTiled;          // a plain-SoA copy, if there is one, is refreshed on its next use
    return HYDRO_OK;
}

int hydro_step_wrench(hydro_t* h, int64_t n, const float* const state[HYDRO_STATE_FIELDS], double dt,
                      float* const wrench[HYDRO_WRENCH_FIELDS], void* stream)
{
    // everything that can be refused is refused BEFORE the engine's plain-SoA previous velocity is allocated and repacked
    int rc = check_soa_step(h, n, state, nullptr, false, dt, wrench);
    if (rc || n == 0) return rc;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if ((rc = prev_acquire(h, hydro_engine::kPrevSoa, n, static_cast<hipStream_t>(stream)))) return rc;   // (allocates the plain copy on first use)
    const PrevRows pv = prev_rows(h);
    return step_soa<true>(h, n, state, pv.f, pv.f, dt, wrench, stream);
}

int hydro_step_wrench_ext(hydro_t* h, int64_t n, const float* const state[HYDRO_STATE_FIELDS],
                          const float* const prev[HYDRO_PREV_FIELDS], double dt,
                          float* const wrench[HYDRO_WRENCH_FIELDS], void* stream)
{
    if (!h) return HYDRO_E_ARG;
    return step_soa<false>(h, n, state, prev, nullptr, dt, wrench, stream);
}

}  // extern "C"

namespace {
// The `time` of the open-loop _sea entries (hydro_step_wrench_tiled_sea, hydro_step_wrench_aos_sea): checked whether or not a
// sea is set.  The kernels take it as sea_water's (step, dt) pair: (double)1 * time == time exactly, and step 0 at time 0.
int check_sea_time(hydro_engine* h, double time)
{
    if (!h) return HYDRO_E_ARG;
    if (!(time >= 0.0) || !(time <= 4503599627370496.0)) return fail(h, HYDRO_E_ARG, "time must be finite, >= 0 and <= 2^52 seconds");
    return HYDRO_OK;
}
inline int64_t sea_step(double time) { return time > 0.0 ? 1 : 0; }
// The launches of the two sea kernels, DEFINED AT THE END OF THIS FILE: a kernel template is emitted where it is first
// instantiated, and these 24 instantiations are to come behind every kernel the library had before them - the existing kernels
// then keep their places in the code object, not only their code.
void launch_wrench_tiled_sea(hydro_engine* h, dim3 grid, dim3 blk, size_t lds, hipStream_t s, const float* state, const float* pv,
                             float* wrench, float* pv_out, uint32_t st_stride, uint32_t pv_stride, uint32_t out_stride, uint32_t pvo_stride,
                             int64_t n, double dt, bool own_prev, double time);
void launch_wrench_aos_sea(hydro_engine* h, hipStream_t s, int64_t n, const float* positions, const float* orientations, int quat_xyzw,
                           const float* velocities, double dt, float* forces, float* torques, double time);

// The open-loop _irr entries (hydro_step_wrench_tiled_irr, hydro_step_wrench_aos_irr): the _sea entries, and the step goes
// through whichever kind of sea the engine holds - the four exclude each other at set time.  What irregular_water finds:
//   table != nullptr : a finite-depth sea (depth), an ensemble, or a lone spectrum as an ensemble of one - tiles_per_sea is then
//                      2^32 - 1, which no tile index reaches, so ensemble_member gives member 0 to every wave
//   table == nullptr : an 8-wave sea or none - the _sea entry's launch
struct IrregularWater { const void* table = nullptr; uint32_t waves = 0, tiles_per_sea = 0; bool depth = false; float neg_depth = 0.0f; };
// 0 and `w` filled, or the refusal of a launch whose LIVE tiles need more members than the table holds (_ens's and _fd's own)
int irregular_water(hydro_engine* h, int64_t n, IrregularWater& w)
{
    const int64_t tiles = (n + HYDRO_TILE - 1) / HYDRO_TILE;
    if (h->fd_waves >= 0) {
        if ((tiles + h->fd_tiles_per_sea - 1) / h->fd_tiles_per_sea > h->fd_count)
            return fail(h, HYDRO_E_ARG, "n needs more members than the finite-depth sea has (count * bodies_per_sea < n)");
        w = IrregularWater{h->fd_table, (uint32_t)h->fd_waves, (uint32_t)h->fd_tiles_per_sea, true, h->fd_neg_depth};
    } else if (h->ensemble_waves >= 0) {
        if ((tiles + h->ensemble_tiles_per_sea - 1) / h->ensemble_tiles_per_sea > h->ensemble_count)
            return fail(h, HYDRO_E_ARG, "n needs more members than the sea ensemble has (count * bodies_per_sea < n)");
        w = IrregularWater{h->ensemble_table, (uint32_t)h->ensemble_waves, (uint32_t)h->ensemble_tiles_per_sea, false, 0.0f};
    } else if (h->spectrum_waves >= 0) {
        w = IrregularWater{h->spectrum_table, (uint32_t)h->spectrum_waves, 0xffffffffu, false, 0.0f};
    }
    return HYDRO_OK;
}
// The launches of the two _irr kernels: defined behind launch_wrench_aos_sea, for the same reason - 48 instantiations that
// come behind every kernel the library had before them.
void launch_wrench_tiled_irr(hydro_engine* h, dim3 grid, dim3 blk, size_t lds, hipStream_t s, const float* state, const float* pv,
                             float* wrench, float* pv_out, uint32_t st_stride, uint32_t pv_stride, uint32_t out_stride, uint32_t pvo_stride,
                             int64_t n, double dt, bool own_prev, double time, const IrregularWater& w);
void launch_wrench_aos_irr(hydro_engine* h, hipStream_t s, int64_t n, const float* positions, const float* orientations, int quat_xyzw,
                           const float* velocities, double dt, float* forces, float* torques, double time, const IrregularWater& w);

// hydro_step_wrench_tiled, optionally sampling the kinetic energy of the state it reads (ke_out != nullptr)
int step_wrench_tiled_impl(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                           const float* prev, int64_t prev_tile_stride, double dt,
                           float* wrench, int64_t wrench_tile_stride, int ke_rotational, double* ke_out, void* stream,
                           const double* sea_time = nullptr, bool irr_entry = false)
{
    // sea_time: the _sea entry - the time is checked first, and the step goes through the sea if one is set
    // irr_entry: the _irr entry - the _sea entry, and a spectrum, an ensemble or a finite-depth sea counts as well
    int rc = sea_time ? check_sea_time(h, *sea_time) : HYDRO_OK;
    if (rc) return rc;
    if ((rc = check_common(h, n))) return rc;
    if (!(dt > 0.0)) return fail(h, HYDRO_E_ARG, "dt must be > 0");
    if ((rc = check_tiled(h, n, state, state_tile_stride, HYDRO_STATE_FIELDS, "null state"))) return rc;
    if ((rc = check_tiled(h, n, wrench, wrench_tile_stride, HYDRO_WRENCH_FIELDS, "null wrench"))) return rc;
    const bool own_prev = (prev == nullptr);
    if (!own_prev && (rc = check_tiled(h, n, prev, prev_tile_stride, HYDRO_PREV_FIELDS, "null prev"))) return rc;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (n == 0) return ke_out ? ke_of_nothing(h, ke_out, static_cast<hipStream_t>(stream)) : HYDRO_OK;
    // the engine's own previous velocity is read, then overwritten with this step's; the caller's is only read
    const float* pv = own_prev ? h->prev_tiled : prev;
    float* pv_out = own_prev ? h->prev_tiled : nullptr;
    const uint32_t pv_stride = own_prev ? HYDRO_PREV_FIELDS * HYDRO_TILE : (uint32_t)prev_tile_stride, pvo_stride = own_prev ? pv_stride : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    IrregularWater irr;                                                     // (the last refusal, before anything is written)
    if (irr_entry && (rc = irregular_water(h, n, irr))) return rc;
    if (own_prev && (rc = prev_acquire(h, hydro_engine::kPrevTiled, n, s))) return rc;
    if (ke_out && (rc = ke_prepare(h, s))) return rc;
    const bool sea = (sea_time && h->sea_waves >= 0) || irr.table;
    const int block = (h->block && !ke_out && !sea) ? h->block : 256;       // (the energy partials are one per 256 bodies; the sea kernels exist for 256 only)
    const dim3 grid(grid_for(n, block)), blk(block);
    // Occupancy shaping: the kernel uses no LDS, so a dynamic-LDS request is a pure residency cap
    // (160 KB per CU / blocks per CU).  Fewer resident waves = fewer DRAM streams in flight.
    const int waves = h->waves < 0 ? 0 : h->waves;
    size_t lds = 0;
    if (waves > 0) {
        const int blocks_per_cu = (waves * 4 * 64) / block;                 // 4 SIMDs x waves x 64 lanes
        lds = blocks_per_cu > 0 ? ((size_t)160 * 1024 / (size_t)blocks_per_cu) & ~(size_t)255 : 0;
        if (lds > 64 * 1024) lds = 64 * 1024;                               // per-block LDS limit
    }
    // ke_out: the sampling variant - same body, same bits, plus one fp64 pair per block and the fixed-order final sum (same
    // launch).  It exists for 256-thread blocks only, which is what `block` is whenever it is asked for.
    if (irr.table) launch_wrench_tiled_irr(h, grid, blk, lds, s, state, pv, wrench, pv_out, (uint32_t)state_tile_stride, pv_stride,
                                           (uint32_t)wrench_tile_stride, pvo_stride, n, dt, own_prev, *sea_time, irr);
    else if (sea) launch_wrench_tiled_sea(h, grid, blk, lds, s, state, pv, wrench, pv_out, (uint32_t)state_tile_stride, pv_stride,
                                     (uint32_t)wrench_tile_stride, pvo_stride, n, dt, own_prev, *sea_time);
    else dispatch_flags([&](auto BIG, auto HALF, auto WP, auto NT, auto KE, auto WARP) {
        if constexpr (BIG || !KE)
            hipLaunchKernelGGL((wrench_tiled_kernel<BIG ? 256 : 128, HALF, WP, NT, KE, WARP>), grid, blk, lds, s,
                               state, pv, h->params_tiled, wrench, pv_out, (uint32_t)state_tile_stride, pv_stride, (uint32_t)wrench_tile_stride, pvo_stride,
                               (uint32_t)n, h->semantics, h->rho, h->g, 1.0 / dt, h->ke_partials, h->ke_stride, ke_rotational, ke_out);
    }, block == 256, h->half_coeffs, own_prev, streaming(h, n), ke_out != nullptr, is_warp(h));
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

// hydro_step_wrench_tiled_batch with a kernarg table of K scenes
template <int K>
void launch_batch(const BatchArgs<K>& table, const hydro_engine* h0, bool own_prev, bool nt, uint32_t blocks, hipStream_t s)
{
    dispatch_flags([&](auto HALF, auto WP, auto NT, auto WARP) {
        hipLaunchKernelGGL((wrench_tiled_batch_kernel<K, HALF, WP, NT, WARP>), dim3(blocks), dim3(kBlock), 0, s, table);
    }, h0->half_coeffs, own_prev, nt, is_warp(h0));
}
}  // namespace

extern "C" {

int hydro_step_wrench_tiled(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                            const float* prev, int64_t prev_tile_stride, double dt,
                            float* wrench, int64_t wrench_tile_stride, void* stream)
{
    return step_wrench_tiled_impl(h, n, state, state_tile_stride, prev, prev_tile_stride, dt, wrench, wrench_tile_stride, 0, nullptr, stream);
}

int hydro_step_wrench_tiled_sea(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                const float* prev, int64_t prev_tile_stride, double dt,
                                float* wrench, int64_t wrench_tile_stride, double time, void* stream)
{
    return step_wrench_tiled_impl(h, n, state, state_tile_stride, prev, prev_tile_stride, dt, wrench, wrench_tile_stride, 0, nullptr, stream, &time);
}

int hydro_step_wrench_tiled_irr(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                const float* prev, int64_t prev_tile_stride, double dt,
                                float* wrench, int64_t wrench_tile_stride, double time, void* stream)
{
    return step_wrench_tiled_impl(h, n, state, state_tile_stride, prev, prev_tile_stride, dt, wrench, wrench_tile_stride, 0, nullptr, stream, &time, true);
}

int hydro_step_wrench_tiled_ke(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                               const float* prev, int64_t prev_tile_stride, double dt,
                               float* wrench, int64_t wrench_tile_stride, int rotational, double* ke_out_dev, void* stream)
{
    if (h && !ke_out_dev) return fail(h, HYDRO_E_ARG, "null ke_out_dev");
    return step_wrench_tiled_impl(h, n, state, state_tile_stride, prev, prev_tile_stride, dt, wrench, wrench_tile_stride,
                                  rotational ? 1 : 0, ke_out_dev, stream);
}

int hydro_step_wrench_tiled_batch(int count, const hydro_scene_t* scenes, double dt, void* stream)
{
    if (count < 1 || count > HYDRO_BATCH_MAX || !scenes || !scenes[0].engine) return HYDRO_E_ARG;
    hydro_engine* h0 = scenes[0].engine;                       // errors are reported on the first scene's handle
    if (!(dt > 0.0)) return fail(h0, HYDRO_E_ARG, "dt must be > 0");
    const bool own_prev = (scenes[0].prev == nullptr);
    BatchArgs<HYDRO_BATCH_MAX> args{};
    int64_t blocks = 0, bodies = 0;
    for (int k = 0; k < HYDRO_BATCH_MAX; ++k) args.first_block[k] = 0xffffffffu;
    for (int k = 0; k < count; ++k) {
        const hydro_scene_t& sc = scenes[k];
        hydro_engine* h = sc.engine;
        if (!h) return fail(h0, HYDRO_E_ARG, "batch: null engine");
        // one kernel instance serves the whole launch: what selects it must be the same for every scene
        if (h->device != h0->device || h->half_coeffs != h0->half_coeffs || h->semantics != h0->semantics || (sc.prev == nullptr) != own_prev)
            return fail(h0, HYDRO_E_ARG, "batch: the scenes of one launch share the device, the coefficient format (f32 / f16), the semantics and "
                                        "the previous-velocity mode (engine-owned or caller-owned)");
        for (int j = 0; j < k; ++j)
            if (scenes[j].engine == h && own_prev) return fail(h0, HYDRO_E_ARG, "batch: an engine that owns the previous velocity may appear once per launch");
        int rc = check_common(h, sc.n);
        if (rc) { if (h != h0) fail(h0, rc, hydro_last_error(h)); return rc; }
        if (sc.n == 0) return fail(h0, HYDRO_E_ARG, "batch: empty scene (leave it out)");
        if ((rc = check_tiled(h, sc.n, sc.state, sc.state_tile_stride, HYDRO_STATE_FIELDS, "null state")) ||
            (rc = check_tiled(h, sc.n, sc.wrench, sc.wrench_tile_stride, HYDRO_WRENCH_FIELDS, "null wrench")) ||
            (!own_prev && (rc = check_tiled(h, sc.n, sc.prev, sc.prev_tile_stride, HYDRO_PREV_FIELDS, "null prev")))) {
            if (h != h0) fail(h0, rc, hydro_last_error(h));
            return rc;
        }
        BatchScene& b = args.sc[k];
        b.st = sc.state; b.st_stride = (uint32_t)sc.state_tile_stride;
        if (own_prev) { b.pv = h->prev_tiled; b.pv_stride = HYDRO_PREV_FIELDS * HYDRO_TILE; b.pv_out = h->prev_tiled; b.pvo_stride = b.pv_stride; }
        else { b.pv = sc.prev; b.pv_stride = (uint32_t)sc.prev_tile_stride; b.pv_out = nullptr; b.pvo_stride = 0; }
        b.prm = h->params_tiled; b.out = sc.wrench; b.out_stride = (uint32_t)sc.wrench_tile_stride;
        b.n = (uint32_t)sc.n; b.pad = 0; b.rho = h->rho; b.g = h->g;
        args.first_block[k] = (uint32_t)blocks;
        blocks += grid_for(sc.n, kBlock);
        bodies += sc.n;
    }
    if (blocks >= ((int64_t)1 << 31)) return fail(h0, HYDRO_E_ARG, "batch: too many bodies for one launch");
    args.inv_dt = 1.0 / dt;
    HYDRO_HIP(h0, use_device(h0->device), HYDRO_E_DEVICE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (own_prev)
        for (int k = 0; k < count; ++k) {
            int rc = prev_acquire(scenes[k].engine, hydro_engine::kPrevTiled, scenes[k].n, s);
            if (rc) return rc;
        }
    const bool nt = streaming(h0, bodies);                      // streaming accesses by the size of the LAUNCH
    if (count <= 4) {                                            // up to four scenes: the short table (see the kernel)
        BatchArgs<4> small{};
        for (int k = 0; k < 4; ++k) { small.first_block[k] = args.first_block[k]; small.sc[k] = args.sc[k < count ? k : 0]; }
        small.inv_dt = args.inv_dt;
        launch_batch(small, h0, own_prev, nt, (uint32_t)blocks, s);
    }
    else launch_batch(args, h0, own_prev, nt, (uint32_t)blocks, s);
    HYDRO_HIP(h0, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int hydro_integrate_tiled(hydro_t* h, int64_t n, const float* state_in, int64_t in_tile_stride,
                          const float* wrench, int64_t wrench_tile_stride, double dt,
                          float* state_out, int64_t out_tile_stride, void* stream)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (!(dt > 0.0)) return fail(h, HYDRO_E_ARG, "dt must be > 0");
    if ((rc = check_tiled(h, n, state_in, in_tile_stride, HYDRO_STATE_FIELDS, "null state_in"))) return rc;
    if ((rc = check_tiled(h, n, wrench, wrench_tile_stride, HYDRO_WRENCH_FIELDS, "null wrench"))) return rc;
    if ((rc = check_tiled(h, n, state_out, out_tile_stride, HYDRO_STATE_FIELDS, "null state_out"))) return rc;
    if (n == 0) return HYDRO_OK;
    IntArgs a;
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) { a.si[f] = state_in + f * HYDRO_TILE; a.so[f] = state_out + f * HYDRO_TILE; }
    for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) a.w[f] = wrench + f * HYDRO_TILE;
    a.si_stride = (uint32_t)in_tile_stride; a.w_stride = (uint32_t)wrench_tile_stride; a.so_stride = (uint32_t)out_tile_stride;
    a.prm = h->params_tiled; a.prm_tile_floats = prm_tile_floats(h); a.mass_field = prm_mass_field(h);
    a.shift = 6; a.mask = 63u; a.g = h->g; a.dt = (float)dt; a.n = (uint32_t)n;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipLaunchKernelGGL(integrate_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

}  // extern "C"

namespace {
// hydro_step_fused_tiled, optionally sampling the kinetic energy of the state it writes (ke_out != nullptr)
int step_fused_tiled_impl(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                          const float* prev, int64_t prev_tile_stride, double dt,
                          float* state_out, int64_t out_tile_stride,
                          float* wrench, int64_t wrench_tile_stride, int implicit_drag, int ke_rotational, double* ke_out, void* stream)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (!(dt > 0.0)) return fail(h, HYDRO_E_ARG, "dt must be > 0");
    if ((rc = check_tiled(h, n, state, state_tile_stride, HYDRO_STATE_FIELDS, "null state"))) return rc;
    if ((rc = check_tiled(h, n, prev, prev_tile_stride, HYDRO_PREV_FIELDS, "null prev (pass the previous state buffer + 7*64)"))) return rc;
    if ((rc = check_tiled(h, n, state_out, out_tile_stride, HYDRO_STATE_FIELDS, "null state_out"))) return rc;
    if (wrench && (rc = check_tiled(h, n, wrench, wrench_tile_stride, HYDRO_WRENCH_FIELDS, "null wrench"))) return rc;
    if (state_out == state) return fail(h, HYDRO_E_ARG, "state_out must not alias state (it may alias the previous-state buffer)");
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) return ke_out ? ke_of_nothing(h, ke_out, s) : HYDRO_OK;
    if (ke_out && (rc = ke_prepare(h, s))) return rc;
    const dim3 grid(grid_for(n, kBlock)), blk(kBlock);
    dispatch_flags([&](auto HALF, auto NT, auto IMPL, auto KE, auto WARP) {
        hipLaunchKernelGGL((step_fused_tiled_kernel<HALF, NT, IMPL, KE, WARP>), grid, blk, 0, s,
                           state, prev, h->params_tiled, state_out, wrench, (uint32_t)state_tile_stride, (uint32_t)prev_tile_stride, (uint32_t)out_tile_stride,
                           wrench ? (uint32_t)wrench_tile_stride : 0u, (uint32_t)n, h->semantics, (float)dt, h->rho, h->g, 1.0 / dt,
                           h->ke_partials, h->ke_stride, ke_rotational, ke_out);
    }, h->half_coeffs, streaming_fused(h, n), implicit_drag != 0, ke_out != nullptr, is_warp(h));
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}
}  // namespace

extern "C" {

int hydro_step_fused_tiled(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                           const float* prev, int64_t prev_tile_stride, double dt,
                           float* state_out, int64_t out_tile_stride,
                           float* wrench, int64_t wrench_tile_stride, int implicit_drag, void* stream)
{
    return step_fused_tiled_impl(h, n, state, state_tile_stride, prev, prev_tile_stride, dt, state_out, out_tile_stride,
                                 wrench, wrench_tile_stride, implicit_drag, 0, nullptr, stream);
}

int hydro_step_fused_tiled_ke(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                              const float* prev, int64_t prev_tile_stride, double dt,
                              float* state_out, int64_t out_tile_stride,
                              float* wrench, int64_t wrench_tile_stride, int implicit_drag,
                              int rotational, double* ke_out_dev, void* stream)
{
    if (h && !ke_out_dev) return fail(h, HYDRO_E_ARG, "null ke_out_dev");
    return step_fused_tiled_impl(h, n, state, state_tile_stride, prev, prev_tile_stride, dt, state_out, out_tile_stride,
                                 wrench, wrench_tile_stride, implicit_drag, rotational ? 1 : 0, ke_out_dev, stream);
}

}  // extern "C"

namespace {

// A launch of any of the seventeen hydro_step_fused_tiled_multi* entries, described ONCE: an entry fills a MultiStep with what it
// was given - the fifteen base members by the braces, every further group by its with_*() below, which is the only place that
// copies the group - and step_fused_tiled_multi_launch validates and launches it.  An option is absent by its pointer
// (log, applied, control, mooring, extremes, tether, tether_peaks: nullptr is "without"); the sea and the seabed are the
// engine's, and an entry that knows of them says so (sea_entry, bed_entry).
struct MultiStep {
    int64_t n; const float* state; int64_t state_tile_stride; const float* prev; int64_t prev_tile_stride; double dt; int steps;
    float* state_out; int64_t out_tile_stride; float* prev_out; int64_t prev_out_tile_stride;
    int implicit_drag, rotational; double* ke_out_dev; void* stream;
    // the recorder, as the entry was given it
    float* log = nullptr; int64_t log_stride = 0, rows_capacity = 0; int fields = HYDRO_STATE_FIELDS, every = 1, phase = 1;
    int64_t row0 = 0; int64_t* rows_written_host = nullptr;
    bool log_required = false;                           // the _rec entry: a null log is refused, and the recorder is checked FIRST
    const float* applied = nullptr; int64_t applied_tile_stride = 0; int applied_frame = HYDRO_FRAME_WORLD;
    const float* control = nullptr; int64_t control_tile_stride = 0;
    bool sea_entry = false; int64_t step0 = 0;           // the _sea entry: step0 is checked, and the steps go through the sea if one is set
    bool bed_entry = false;                              // the _bed entry: the _sea entry, and the steps meet the seabed if one is set
    bool irr_entry = false;                              // the _irr entry: the _spread entry, and the steps go through the sea spectrum if one is set
    const float* mooring = nullptr; int64_t mooring_tile_stride = 0;      // the _moor entry: the _bed entry, and a line per body if a record is given
    float* extremes = nullptr; int64_t extremes_tile_stride = 0;          // the _ext entry: the _moor entry, and the running extremes if a record is given
    const float* tether = nullptr; int64_t tether_tile_stride = 0;        // the _teth entry: the _ext entry, and a line between two bodies of a tile if a record is given
    int64_t tether_layers = 0;                           // the _net entry: the _teth entry with `tether` a net of that many layers (0: a single record, the _teth entry's)
    float* tether_peaks = nullptr; int64_t tether_peaks_tile_stride = 0;  // the _peak entry: the _net entry, and the running maximum of every line's tension if a record is given
    int64_t mooring_layers = 0;                          // the _spread entry: the _peak entry with `mooring` a spread of that many layers (0: a single record, the _moor entry's)
    // the _stat entry: the _irr entry, and the running response statistics if a record is given
    bool stat_entry = false; void* statistics = nullptr; int64_t statistics_tile_stride = 0;
    const float* levels = nullptr; int64_t levels_tile_stride = 0; int channel_a = 0, channel_b = 0;
    bool ens_entry = false;                              // the _ens entry: the _stat entry, and block m of the bodies steps through member m of the sea ensemble if one is set
    bool fd_entry = false;                               // the _fd entry: the _ens entry, and the finite-depth sea's water if one is set

    void with_recorder(float* log_, int64_t log_stride_, int64_t rows_capacity_, int fields_, int every_, int phase_, int64_t row0_, int64_t* rows_written_host_)
    {
        log = log_; log_stride = log_stride_; rows_capacity = rows_capacity_; fields = fields_; every = every_; phase = phase_;
        row0 = row0_; rows_written_host = rows_written_host_;
    }
    void with_applied(const float* p, int64_t stride, int frame) { applied = p; applied_tile_stride = stride; applied_frame = frame; }
    void with_control(const float* p, int64_t stride) { control = p; control_tile_stride = stride; }
    void with_sea(int64_t step0_) { sea_entry = true; step0 = step0_; }
    void with_seabed() { bed_entry = true; }
    void with_spectrum() { irr_entry = true; }
    void with_mooring(const float* p, int64_t stride) { mooring = p; mooring_tile_stride = stride; }
    void with_extremes(float* p, int64_t stride) { extremes = p; extremes_tile_stride = stride; }
    void with_tether(const float* p, int64_t stride) { tether = p; tether_tile_stride = stride; }
    // (a net of no layers is none of the launch's forms: it is refused as out of range, never taken for the _teth entry's record)
    void with_layers(int64_t layers) { tether_layers = layers == 0 ? -1 : layers; }
    void with_peaks(float* p, int64_t stride) { tether_peaks = p; tether_peaks_tile_stride = stride; }
    // (a spread of no layers is refused as out of range, never taken for the _moor entry's record)
    void with_mooring_layers(int64_t layers) { mooring_layers = layers == 0 ? -1 : layers; }
    void with_statistics(void* p, int64_t stride, const float* levels_, int64_t levels_stride, int a, int b)
    {
        stat_entry = true; statistics = p; statistics_tile_stride = stride; levels = levels_; levels_tile_stride = levels_stride;
        channel_a = a; channel_b = b;
    }
    void with_ensemble() { ens_entry = true; }
    void with_finite_depth() { fd_entry = true; }
    bool shear_entry = false;                            // the _shear entry: the _fd entry, and the current profile's water if one is set
    void with_current_profile() { shear_entry = true; }
};
// [p, p + floats) and [q, q + floats_q) share an element
inline bool ranges_overlap(const float* p, int64_t floats, const float* q, int64_t floats_q)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)floats_q * 4u && b < a + (uintptr_t)floats * 4u;
}
// floats from the first to the last field of `fields`-field records in `tiles` tiles: what a kernel touches of an output.
// (prev_out is usually the velocity fields INSIDE a state buffer: tiles * stride would reach 7 * 64 floats past its end,
// into whatever the allocator put there)
inline int64_t tiled_extent(int64_t tiles, int64_t stride, int fields)
{
    return tiles > 0 ? (tiles - 1) * stride + (int64_t)fields * HYDRO_TILE : 0;
}
// A per-body input record (`what`: "applied" / "control" / "mooring"; `stride` floats per tile) must lie outside everything the launch writes.
int check_no_overlap(hydro_t* h, const MultiStep& m, int64_t log_floats, const char* what, const float* p, int64_t stride)
{
    const int64_t tiles = (m.n + HYDRO_TILE - 1) / HYDRO_TILE, floats = tiles * stride;
    if (!ranges_overlap(p, floats, m.state_out, tiled_extent(tiles, m.out_tile_stride, HYDRO_STATE_FIELDS))
        && !ranges_overlap(p, floats, m.prev_out, tiled_extent(tiles, m.prev_out_tile_stride, HYDRO_PREV_FIELDS))
        && !(m.log && ranges_overlap(p, floats, m.log, log_floats)))
        return HYDRO_OK;
    char msg[96];
    snprintf(msg, sizeof msg, "%s must not overlap an output (state_out, prev_out, log)", what);
    return fail(h, HYDRO_E_ARG, msg);
}

// What a recording launch checks of its recorder arguments; `rows`: the rows the launch writes.
int check_recorder(hydro_t* h, const MultiStep& m, int64_t& rows_out)
{
    if (h->watch_count == 0) return fail(h, HYDRO_E_STATE, "no watch list (call hydro_set_watch first)");
    if (!m.log || !aligned_to(m.log, 4)) return fail(h, HYDRO_E_ARG, "null or misaligned log");
    if (m.fields != HYDRO_STATE_FIELDS && m.fields != HYDRO_STATE_FIELDS + HYDRO_WRENCH_FIELDS) return fail(h, HYDRO_E_ARG, "fields must be 13 (state) or 19 (state + wrench)");
    if (m.every < 1 || m.every > (1 << 30)) return fail(h, HYDRO_E_ARG, "every must be in 1 .. 2^30");
    if (m.phase < 1 || m.phase > m.every) return fail(h, HYDRO_E_ARG, "phase must be in 1 .. every");
    if (m.log_stride < h->watch_count || m.log_stride >= ((int64_t)1 << 31)) return fail(h, HYDRO_E_ARG, "log_stride must be >= the watch count (and < 2^31)");
    if (m.row0 < 0 || m.rows_capacity < 0 || m.rows_capacity >= ((int64_t)1 << 31)) return fail(h, HYDRO_E_ARG, "row0 / rows_capacity out of range (0 .. 2^31)");
    if (m.steps < 1 || m.steps > (1 << 20)) return fail(h, HYDRO_E_ARG, "steps must be in 1 .. 2^20");
    // the rows this launch writes: row0 .. row0 + rows - 1, all of them below rows_capacity before anything is launched
    const int64_t rows = rows_out = m.phase > m.steps ? 0 : (int64_t)(m.steps - m.phase) / m.every + 1;
    if (rows > 0 && m.row0 + rows > m.rows_capacity) return fail(h, HYDRO_E_ARG, "the launch would write past rows_capacity");
    return HYDRO_OK;
}

// The refusals in the order the entries have always reported them, then ONE choice of kernel family.  The families form a
// ladder, each taking its predecessor's argument groups and one more:
//   plain < _rec < _app < _ctl < _sea < _bed < _moor < _ext < _teth < _net < _peak < _spread
// (the _irr family stands beside the ladder: it is chosen while a sea spectrum is set, by the _irr entry alone, whatever the options;
// the two _stat families stand beside the _spread and the _irr family: chosen while a statistics record is given, whatever the options;
// the two _ens families stand beside the _irr and the _irr_stat family: chosen while a sea ensemble is set, by the _ens entry alone;
// the two _fd families stand beside the two _ens families: chosen while a finite-depth sea is set, by the _fd entry alone;
// the two _shear families stand beside the two _fd families: chosen while a current profile AND a finite-depth sea are set, by the _shear entry alone)
// and a launch goes to the LOWEST family that takes every option it has (the higher ones compute the same bits, slower for
// the lesser cases); the options below the chosen one that the launch goes without are handed over as absent ones.
int step_fused_tiled_multi_launch(hydro_t* h, const MultiStep& m)
{
    if (!h) return HYDRO_E_ARG;
    int rc;
    if (m.sea_entry && (m.step0 < 0 || m.steps < 0 || m.step0 + (int64_t)m.steps >= ((int64_t)1 << 52) || m.step0 >= ((int64_t)1 << 52)))
        return fail(h, HYDRO_E_ARG, "step0 must be >= 0 and step0 + steps < 2^52");
    const bool rec = m.log || m.log_required, sea = m.sea_entry && h->sea_waves >= 0, bed = m.bed_entry && h->has_bed;
    const bool irr = m.irr_entry && h->spectrum_waves >= 0;                    // (a spectrum and a sea are never set together: irr implies !sea)
    const bool ens = m.ens_entry && h->ensemble_waves >= 0;                    // (nor an ensemble with either: ens implies !irr and !sea)
    const bool fd = m.fd_entry && h->fd_waves >= 0;                            // (nor a finite-depth sea with any of them: fd implies !ens, !irr and !sea)
    const bool shear = m.shear_entry && h->shear_knots > 0;                    // (a profile needs a water column: refused below without fd)
    int64_t rows = 0;
    if (rec && (rc = check_recorder(h, m, rows))) return rc;
    if ((rc = check_common(h, m.n))) return rc;
    if (!(m.dt > 0.0)) return fail(h, HYDRO_E_ARG, "dt must be > 0");
    if (m.steps < 1 || m.steps > (1 << 20)) return fail(h, HYDRO_E_ARG, "steps must be in 1 .. 2^20");
    if ((rc = check_tiled(h, m.n, m.state, m.state_tile_stride, HYDRO_STATE_FIELDS, "null state"))) return rc;
    if ((rc = check_tiled(h, m.n, m.prev, m.prev_tile_stride, HYDRO_PREV_FIELDS, "null prev (pass the previous state buffer + 7*64)"))) return rc;
    if ((rc = check_tiled(h, m.n, m.state_out, m.out_tile_stride, HYDRO_STATE_FIELDS, "null state_out"))) return rc;
    if ((rc = check_tiled(h, m.n, m.prev_out, m.prev_out_tile_stride, HYDRO_PREV_FIELDS, "null prev_out (pass state + 7*64 to keep the two-buffer ping-pong)"))) return rc;
    if (m.state_out == m.state) return fail(h, HYDRO_E_ARG, "state_out must not alias state (it may alias the previous-state buffer)");
    if (rec && h->watch_last >= m.n) return fail(h, HYDRO_E_ARG, "a watched body is >= n");
    const int64_t log_floats = m.log ? m.rows_capacity * m.fields * m.log_stride : 0;      // the log as an output range the inputs must stay out of
    if (m.applied) {
        if ((rc = check_tiled(h, m.n, m.applied, m.applied_tile_stride, HYDRO_WRENCH_FIELDS, "null applied"))) return rc;
        if (m.applied_frame != HYDRO_FRAME_WORLD && m.applied_frame != HYDRO_FRAME_BODY) return fail(h, HYDRO_E_ARG, "applied_frame must be HYDRO_FRAME_WORLD or HYDRO_FRAME_BODY");
        if ((rc = check_no_overlap(h, m, log_floats, "applied", m.applied, m.applied_tile_stride))) return rc;
    }
    if (m.control) {
        if ((rc = check_tiled(h, m.n, m.control, m.control_tile_stride, HYDRO_CTL_FIELDS, "null control"))) return rc;
        if ((rc = check_no_overlap(h, m, log_floats, "control", m.control, m.control_tile_stride))) return rc;
    }
    if (m.mooring) {
        if ((rc = check_tiled(h, m.n, m.mooring, m.mooring_tile_stride, HYDRO_MOOR_FIELDS, "null mooring"))) return rc;
        if ((rc = check_no_overlap(h, m, log_floats, "mooring", m.mooring, m.mooring_tile_stride))) return rc;
    }
    if (m.extremes) {
        if ((rc = check_tiled(h, m.n, m.extremes, m.extremes_tile_stride, HYDRO_EXT_FIELDS, "null extremes"))) return rc;
        if ((rc = check_no_overlap(h, m, log_floats, "extremes", m.extremes, m.extremes_tile_stride))) return rc;
        // it is written: it must stay out of what the launch reads as well
        const int64_t tiles = (m.n + HYDRO_TILE - 1) / HYDRO_TILE, floats = tiled_extent(tiles, m.extremes_tile_stride, HYDRO_EXT_FIELDS);
        const auto reads = [&](const float* p, int64_t stride, int fields) {
            return p && ranges_overlap(m.extremes, floats, p, tiled_extent(tiles, stride, fields));
        };
        if (reads(m.state, m.state_tile_stride, HYDRO_STATE_FIELDS) || reads(m.prev, m.prev_tile_stride, HYDRO_PREV_FIELDS)
            || reads(m.applied, m.applied_tile_stride, HYDRO_WRENCH_FIELDS) || reads(m.control, m.control_tile_stride, HYDRO_CTL_FIELDS)
            || reads(m.mooring, m.mooring_tile_stride, HYDRO_MOOR_FIELDS))
            return fail(h, HYDRO_E_ARG, "extremes must not overlap an input (state, prev, applied, control, mooring)");
    }
    if (m.tether) {
        if (m.tether_layers != 0 && (m.tether_layers < 1 || m.tether_layers > HYDRO_TETH_LAYERS_MAX))            // (0: not the _net entry)
            return fail(h, HYDRO_E_ARG, "tether_layers must be in 1 .. HYDRO_TETH_LAYERS_MAX");
        if ((rc = check_tiled(h, m.n, m.tether, m.tether_tile_stride, HYDRO_TETH_FIELDS * (m.tether_layers ? (int)m.tether_layers : 1), "null tether"))) return rc;
        if ((rc = check_no_overlap(h, m, log_floats, "tether", m.tether, m.tether_tile_stride))) return rc;
        const int64_t tiles = (m.n + HYDRO_TILE - 1) / HYDRO_TILE;                 // the extremes record is an output too
        if (m.extremes && ranges_overlap(m.tether, tiles * m.tether_tile_stride, m.extremes, tiled_extent(tiles, m.extremes_tile_stride, HYDRO_EXT_FIELDS)))
            return fail(h, HYDRO_E_ARG, "tether must not overlap an output (extremes)");
    }
    if (m.tether_peaks) {
        if (!m.tether) return fail(h, HYDRO_E_ARG, "tether_peaks without a tether net");
        const int layers = (int)m.tether_layers;                                   // (the _peak entry is a _net entry: 1 .. 4 by now)
        if ((rc = check_tiled(h, m.n, m.tether_peaks, m.tether_peaks_tile_stride, layers, "null tether_peaks"))) return rc;
        // it is written in every step: it must stay out of everything else the launch reads or writes
        const int64_t tiles = (m.n + HYDRO_TILE - 1) / HYDRO_TILE, floats = tiled_extent(tiles, m.tether_peaks_tile_stride, layers);
        const auto meets = [&](const float* p, int64_t stride, int fields) {
            return p && ranges_overlap(m.tether_peaks, floats, p, tiled_extent(tiles, stride, fields));
        };
        if (meets(m.state_out, m.out_tile_stride, HYDRO_STATE_FIELDS) || meets(m.prev_out, m.prev_out_tile_stride, HYDRO_PREV_FIELDS)
            || meets(m.state, m.state_tile_stride, HYDRO_STATE_FIELDS) || meets(m.prev, m.prev_tile_stride, HYDRO_PREV_FIELDS)
            || meets(m.applied, m.applied_tile_stride, HYDRO_WRENCH_FIELDS) || meets(m.control, m.control_tile_stride, HYDRO_CTL_FIELDS)
            || meets(m.mooring, m.mooring_tile_stride, HYDRO_MOOR_FIELDS) || meets(m.tether, m.tether_tile_stride, HYDRO_TETH_FIELDS * layers)
            || meets(m.extremes, m.extremes_tile_stride, HYDRO_EXT_FIELDS) || (m.log && ranges_overlap(m.tether_peaks, floats, m.log, log_floats)))
            return fail(h, HYDRO_E_ARG, "tether_peaks must not overlap an output, an input record, the net, the extremes or the log");
    }
    if (m.mooring && m.mooring_layers != 0) {
        // the _spread entry: the record has passed as a single line's (its layer 0 is one) - now as the spread it is
        if (m.mooring_layers < 1 || m.mooring_layers > HYDRO_MOOR_LAYERS_MAX) return fail(h, HYDRO_E_ARG, "mooring_layers must be in 1 .. HYDRO_MOOR_LAYERS_MAX");
        const int fields = HYDRO_MOOR_FIELDS * (int)m.mooring_layers;
        if ((rc = check_tiled(h, m.n, m.mooring, m.mooring_tile_stride, fields, "null mooring"))) return rc;
        const int64_t tiles = (m.n + HYDRO_TILE - 1) / HYDRO_TILE, floats = tiled_extent(tiles, m.mooring_tile_stride, fields);
        const auto written = [&](const float* p, int64_t stride, int f) {
            return p && ranges_overlap(m.mooring, floats, p, tiled_extent(tiles, stride, f));
        };
        if (written(m.state_out, m.out_tile_stride, HYDRO_STATE_FIELDS) || written(m.prev_out, m.prev_out_tile_stride, HYDRO_PREV_FIELDS)
            || written(m.extremes, m.extremes_tile_stride, HYDRO_EXT_FIELDS)
            || (m.tether_peaks && written(m.tether_peaks, m.tether_peaks_tile_stride, (int)m.tether_layers))
            || (m.log && ranges_overlap(m.mooring, floats, m.log, log_floats)))
            return fail(h, HYDRO_E_ARG, "the mooring spread must not overlap an output (state_out, prev_out, log, extremes, tether_peaks)");
    }
    if (m.stat_entry) {
        if (m.channel_a < 0 || m.channel_a >= HYDRO_STAT_CHANNELS || m.channel_b < 0 || m.channel_b >= HYDRO_STAT_CHANNELS)
            return fail(h, HYDRO_E_ARG, "channel_a / channel_b must be in 0 .. 6 (HYDRO_STAT_X .. HYDRO_STAT_TENSION)");
    }
    if (m.statistics) {
        constexpr int kStatFloats = HYDRO_STAT_BYTES_PER_BODY / 4;                 // the record in 4-byte units per body: what check_tiled counts
        if (!m.levels) return fail(h, HYDRO_E_ARG, "null levels (a statistics record needs its level record)");
        if ((rc = check_tiled(h, m.n, m.statistics, m.statistics_tile_stride, kStatFloats, "null statistics"))) return rc;
        if ((rc = check_tiled(h, m.n, m.levels, m.levels_tile_stride, HYDRO_STAT_LEVEL_FIELDS, "null levels"))) return rc;
        const int64_t tiles = (m.n + HYDRO_TILE - 1) / HYDRO_TILE;
        const float* st = static_cast<const float*>(m.statistics);
        const int64_t st_floats = tiled_extent(tiles, m.statistics_tile_stride, kStatFloats), lv_floats = tiled_extent(tiles, m.levels_tile_stride, HYDRO_STAT_LEVEL_FIELDS);
        const int net_fields = HYDRO_TETH_FIELDS * (m.tether_layers > 0 ? (int)m.tether_layers : 1), peak_fields = m.tether_layers > 0 ? (int)m.tether_layers : 1;
        const int moor_fields = HYDRO_MOOR_FIELDS * (m.mooring_layers > 0 ? (int)m.mooring_layers : 1);
        const auto meets = [&](const float* q, int64_t q_floats, const void* p, int64_t stride, int fields) {
            return p && ranges_overlap(q, q_floats, static_cast<const float*>(p), tiled_extent(tiles, stride, fields));
        };
        const auto meets_output = [&](const float* q, int64_t q_floats) {
            return meets(q, q_floats, m.state_out, m.out_tile_stride, HYDRO_STATE_FIELDS) || meets(q, q_floats, m.prev_out, m.prev_out_tile_stride, HYDRO_PREV_FIELDS)
                || meets(q, q_floats, m.extremes, m.extremes_tile_stride, HYDRO_EXT_FIELDS) || meets(q, q_floats, m.tether_peaks, m.tether_peaks_tile_stride, peak_fields)
                || (m.log && ranges_overlap(q, q_floats, m.log, log_floats));
        };
        if (meets_output(st, st_floats))
            return fail(h, HYDRO_E_ARG, "statistics must not overlap an output (state_out, prev_out, log, extremes, tether_peaks)");
        if (meets(st, st_floats, m.state, m.state_tile_stride, HYDRO_STATE_FIELDS) || meets(st, st_floats, m.prev, m.prev_tile_stride, HYDRO_PREV_FIELDS)
            || meets(st, st_floats, m.applied, m.applied_tile_stride, HYDRO_WRENCH_FIELDS) || meets(st, st_floats, m.control, m.control_tile_stride, HYDRO_CTL_FIELDS)
            || meets(st, st_floats, m.mooring, m.mooring_tile_stride, moor_fields) || meets(st, st_floats, m.tether, m.tether_tile_stride, net_fields)
            || meets(st, st_floats, m.levels, m.levels_tile_stride, HYDRO_STAT_LEVEL_FIELDS))
            return fail(h, HYDRO_E_ARG, "statistics must not overlap an input (state, prev, applied, control, mooring, tether, levels)");
        if (meets_output(m.levels, lv_floats))
            return fail(h, HYDRO_E_ARG, "levels must not overlap an output (state_out, prev_out, log, extremes, tether_peaks)");
    }
    if (ens) {
        // the last refusal: every LIVE tile's member must be in the table (the kernels index it by tile / tiles_per_sea, unchecked)
        const int64_t tiles = (m.n + HYDRO_TILE - 1) / HYDRO_TILE;
        if ((tiles + h->ensemble_tiles_per_sea - 1) / h->ensemble_tiles_per_sea > h->ensemble_count)
            return fail(h, HYDRO_E_ARG, "n needs more members than the sea ensemble has (count * bodies_per_sea < n)");
    }
    if (fd) {
        const int64_t tiles = (m.n + HYDRO_TILE - 1) / HYDRO_TILE;
        if ((tiles + h->fd_tiles_per_sea - 1) / h->fd_tiles_per_sea > h->fd_count)
            return fail(h, HYDRO_E_ARG, "n needs more members than the finite-depth sea has (count * bodies_per_sea < n)");
    }
    if (shear && !fd)
        return fail(h, HYDRO_E_STATE, "a current profile is set without a finite-depth sea (call hydro_set_sea_finite_depth first, or clear the profile: hydro_set_current_profile(h, NULL))");
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipStream_t s = static_cast<hipStream_t>(m.stream);
    if (m.rows_written_host) *m.rows_written_host = m.n == 0 ? 0 : rows;
    if (m.n == 0) return m.ke_out_dev ? ke_of_nothing(h, m.ke_out_dev, s) : HYDRO_OK;
    const dim3 grid(grid_for(m.n, kBlock)), blk(kBlock);
    if (m.ke_out_dev && (rc = ke_prepare(h, s))) return rc;
    // the kernels' recorder arguments: the engine's watch tables and the log, or the absent recorder
    struct Recorder { const uint64_t* mask; const uint32_t* first; float* log; uint32_t stride, fields, every, phase, row0; };
    const Recorder none = {nullptr, nullptr, nullptr, 0u, (uint32_t)HYDRO_STATE_FIELDS, 1u, 1u, 0u};
    const Recorder r = !rec ? none : Recorder{h->watch_mask, h->watch_first, m.log, (uint32_t)m.log_stride, (uint32_t)m.fields,
                                              (uint32_t)m.every, (uint32_t)m.phase, (uint32_t)m.row0};
    const uint32_t applied_stride = m.applied ? (uint32_t)m.applied_tile_stride : 0u, control_stride = m.control ? (uint32_t)m.control_tile_stride : 0u;
    const int frame = m.applied ? m.applied_frame : HYDRO_FRAME_WORLD;
    dispatch_flags([&](auto HALF, auto NT, auto IMPL, auto KE, auto WARP) {
        // One link per argument group, in the kernels' order (HYDRO_*_PARAMS): a link hands its group on to the link below it and
        // whatever the links above it gave behind that, so a group's expressions stand here once.  Where an argument depends on
        // its option being there (`sea ? table : null`, `m.mooring ? stride : 0`), the family that is chosen BECAUSE the option is
        // there finds the condition true and gets the option's own values: the conditional form is exact for every family.
        const auto plain = [&](auto kernel, auto... tail) {
            hipLaunchKernelGGL(kernel, grid, blk, 0, s, m.state, m.prev, h->params_tiled, m.state_out, m.prev_out,
                               (uint32_t)m.state_tile_stride, (uint32_t)m.prev_tile_stride, (uint32_t)m.out_tile_stride, (uint32_t)m.prev_out_tile_stride,
                               (uint32_t)m.n, (uint32_t)m.steps, (float)m.dt, h->rho, h->g, 1.0 / m.dt, h->ke_partials, h->ke_stride, m.rotational ? 1 : 0, m.ke_out_dev,
                               tail...);
        };
        const auto recording = [&](auto kernel, auto... tail) { plain(kernel, r.mask, r.first, r.log, r.stride, r.fields, r.every, r.phase, r.row0, tail...); };
        const auto pushed = [&](auto kernel, auto... tail) { recording(kernel, m.applied, applied_stride, frame, tail...); };
        const auto held = [&](auto kernel, auto... tail) { pushed(kernel, m.control, control_stride, tail...); };
        const auto in_sea = [&](auto kernel, auto... tail) {
            held(kernel, fd ? (const void*)h->fd_table : ens ? (const void*)h->ensemble_table : irr ? (const void*)h->spectrum_table : sea ? (const void*)h->sea_table : (const void*)nullptr,
                 fd ? (uint32_t)h->fd_waves : ens ? (uint32_t)h->ensemble_waves : irr ? (uint32_t)h->spectrum_waves : sea ? (uint32_t)h->sea_waves : 0u, m.step0, m.dt, tail...);
        };
        const auto on_bed = [&](auto kernel, auto... tail) {
            in_sea(kernel, h->bed.z, h->bed.stiffness, h->bed.damping, h->bed.friction, h->bed.slip_speed, h->bed.friction_rate, tail...);
        };
        const auto on_optional_bed = [&](auto kernel, auto... tail) { on_bed(kernel, bed ? 1 : 0, tail...); };
        const auto moored = [&](auto kernel, auto... tail) { on_optional_bed(kernel, m.mooring, m.mooring ? (uint32_t)m.mooring_tile_stride : 0u, tail...); };
        const auto tracked = [&](auto kernel, auto... tail) { moored(kernel, m.extremes, m.extremes ? (uint32_t)m.extremes_tile_stride : 0u, tail...); };
        const auto tethered = [&](auto kernel, auto... tail) { tracked(kernel, m.tether, (uint32_t)m.tether_tile_stride, tail...); };
        const auto netted = [&](auto kernel, auto... tail) { tethered(kernel, (uint32_t)m.tether_layers, tail...); };
        // (the spread's layer count stands behind the mooring group, in front of the groups that follow it: its link takes them as its tail)
        const auto spread_moored = [&](auto kernel, auto... tail) {
            on_optional_bed(kernel, m.mooring, m.mooring ? (uint32_t)m.mooring_tile_stride : 0u, m.mooring ? (uint32_t)m.mooring_layers : 0u, tail...);
        };
        // (the _spread family's groups behind the spread, every one optional: the _irr family takes them unchanged)
        const auto spread_and_all = [&](auto kernel, auto... tail) {
            spread_moored(kernel, m.extremes, m.extremes ? (uint32_t)m.extremes_tile_stride : 0u,
                          m.tether, m.tether ? (uint32_t)m.tether_tile_stride : 0u, m.tether ? (uint32_t)(m.tether_layers ? m.tether_layers : 1) : 0u,
                          m.tether_peaks, m.tether_peaks ? (uint32_t)m.tether_peaks_tile_stride : 0u, tail...);
        };
        // (the statistics group behind everything else: the two _stat families take the _spread family's groups unchanged)
        const auto with_statistics = [&](auto kernel, auto... tail) {
            spread_and_all(kernel, m.statistics, (uint32_t)m.statistics_tile_stride, m.levels, (uint32_t)m.levels_tile_stride, (uint32_t)m.channel_a, (uint32_t)m.channel_b, tail...);
        };
        // the current profile first: the finite-depth sea's groups and the knot table behind everything else; then
        // the finite-depth sea: the ensemble's group and the depth behind everything else, every option the launch has; then
        // the ensemble: its group stands behind everything else, and its two families take every option the launch has; then
        // the statistics, through the spectrum or not; then
        // the spectrum: its family stands beside the ladder, not on it, and takes every option the launch has
        if (shear) {
            const uint32_t tiles_per_sea = (uint32_t)h->fd_tiles_per_sea, knots = (uint32_t)h->shear_knots;
            if (m.statistics) with_statistics(step_fused_multi_shear_stat_tiled_kernel<HALF, NT, IMPL, KE, WARP>, tiles_per_sea, h->fd_neg_depth, (const void*)h->shear_table, knots);
            else spread_and_all(step_fused_multi_shear_tiled_kernel<HALF, NT, IMPL, KE, WARP>, tiles_per_sea, h->fd_neg_depth, (const void*)h->shear_table, knots);
        }
        else if (fd) {
            const uint32_t tiles_per_sea = (uint32_t)h->fd_tiles_per_sea;
            if (m.statistics) with_statistics(step_fused_multi_fd_stat_tiled_kernel<HALF, NT, IMPL, KE, WARP>, tiles_per_sea, h->fd_neg_depth);
            else spread_and_all(step_fused_multi_fd_tiled_kernel<HALF, NT, IMPL, KE, WARP>, tiles_per_sea, h->fd_neg_depth);
        }
        else if (ens) {
            const uint32_t tiles_per_sea = (uint32_t)h->ensemble_tiles_per_sea;
            if (m.statistics) with_statistics(step_fused_multi_ens_stat_tiled_kernel<HALF, NT, IMPL, KE, WARP>, tiles_per_sea);
            else spread_and_all(step_fused_multi_ens_tiled_kernel<HALF, NT, IMPL, KE, WARP>, tiles_per_sea);
        }
        else if (m.statistics) {
            if (irr) with_statistics(step_fused_multi_irr_stat_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
            else with_statistics(step_fused_multi_stat_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        }
        else if (irr) spread_and_all(step_fused_multi_irr_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else if (m.mooring && m.mooring_layers) spread_and_all(step_fused_multi_spread_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else if (m.tether_peaks) netted(step_fused_multi_peak_tiled_kernel<HALF, NT, IMPL, KE, WARP>, m.tether_peaks, (uint32_t)m.tether_peaks_tile_stride);
        else if (m.tether && m.tether_layers) netted(step_fused_multi_net_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else if (m.tether) tethered(step_fused_multi_teth_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else if (m.extremes) tracked(step_fused_multi_ext_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else if (m.mooring) moored(step_fused_multi_moor_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else if (bed) on_bed(step_fused_multi_bed_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else if (sea) in_sea(step_fused_multi_sea_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else if (m.control) held(step_fused_multi_ctl_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else if (m.applied) pushed(step_fused_multi_app_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else if (rec) recording(step_fused_multi_rec_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
        else plain(step_fused_multi_tiled_kernel<HALF, NT, IMPL, KE, WARP>);
    }, h->half_coeffs, streaming_fused(h, m.n), m.implicit_drag != 0, m.ke_out_dev != nullptr, is_warp(h));
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

}  // namespace

extern "C" {

int hydro_step_fused_tiled_multi(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                 const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                 float* state_out, int64_t out_tile_stride,
                                 float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                 int rotational, double* ke_out_dev, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_set_watch(hydro_t* h, int64_t count, const int64_t* bodies_host)
{
    if (!h) return HYDRO_E_ARG;
    if (count == 0 || !bodies_host) {
        if (count > 0) return fail(h, HYDRO_E_ARG, "null watch list with count > 0");
        if (count < 0) return fail(h, HYDRO_E_ARG, "watch list: count < 0");
        h->watch_count = 0;
        h->watch_last = -1;
        return HYDRO_OK;
    }
    switch (hydro::watch_check(count, bodies_host, h->capacity)) {
        case 0: break;
        case 1: return fail(h, HYDRO_E_ARG, "watch list: count out of range (0 .. HYDRO_WATCH_MAX)");
        case 2: return fail(h, HYDRO_E_ARG, "watch list: body index out of range (0 <= body < capacity)");
        default: return fail(h, HYDRO_E_ARG, "watch list: indices must be strictly ascending (sorted, no duplicates)");
    }
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    const size_t tiles = (size_t)((h->capacity + HYDRO_TILE - 1) / HYDRO_TILE);
    if (!h->watch_mask && hipMalloc(&h->watch_mask, tiles * sizeof(uint64_t)) != hipSuccess) { h->watch_mask = nullptr; return fail(h, HYDRO_E_ALLOC, "watch tables: allocation failed"); }
    if (!h->watch_first && hipMalloc(&h->watch_first, tiles * sizeof(uint32_t)) != hipSuccess) { h->watch_first = nullptr; return fail(h, HYDRO_E_ALLOC, "watch tables: allocation failed"); }
    uint64_t* mask = static_cast<uint64_t*>(malloc(tiles * sizeof(uint64_t)));
    uint32_t* first = static_cast<uint32_t*>(malloc(tiles * sizeof(uint32_t)));
    if (!mask || !first) { free(mask); free(first); return fail(h, HYDRO_E_ALLOC, "watch tables: host allocation failed"); }
    hydro::watch_tables(count, bodies_host, (int64_t)tiles, mask, first);
    // from here on the device tables are being rewritten: a failure leaves NO list, never half of one
    h->watch_count = 0;
    h->watch_last = -1;
    hipError_t e = hipMemcpyAsync(h->watch_mask, mask, tiles * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->watch_first, first, tiles * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    free(mask);
    free(first);
    if (e != hipSuccess) return fail(h, HYDRO_E_LAUNCH, "watch tables: copy to the device", e);
    h->watch_count = count;
    h->watch_last = bodies_host[count - 1];
    return HYDRO_OK;
}

int64_t hydro_watch_count(const hydro_t* h) { return h ? h->watch_count : 0; }

int hydro_step_fused_tiled_multi_rec(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                     const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                     float* state_out, int64_t out_tile_stride,
                                     float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double* ke_out_dev,
                                     float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t* rows_written_host, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.log_required = true;
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_step_fused_tiled_multi_app(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                     const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                     float* state_out, int64_t out_tile_stride,
                                     float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double* ke_out_dev,
                                     float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t* rows_written_host,
                                     const float* applied, int64_t applied_tile_stride, int applied_frame, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_step_fused_tiled_multi_ctl(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                     const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                     float* state_out, int64_t out_tile_stride,
                                     float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double* ke_out_dev,
                                     float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t* rows_written_host,
                                     const float* applied, int64_t applied_tile_stride, int applied_frame,
                                     const float* control, int64_t control_tile_stride, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    return step_fused_tiled_multi_launch(h, m);
}

}  // extern "C"

namespace {
// What hydro_set_sea and hydro_set_sea_spectrum check of a sea and how they form its device records: `u` and `out[0 .. waves)`
// (zeroed by the caller).  `what` ("sea" / "sea spectrum") heads the messages.
int sea_records(hydro_t* h, const char* what, const double (&current)[3], int waves, const hydro_sea_wave_t* wave, float (&u)[3], SeaWave* out)
{
    char msg[128];
    const auto refuse = [&](const char* why) { snprintf(msg, sizeof msg, "%s: %s", what, why); return fail(h, HYDRO_E_ARG, msg); };
    for (int i = 0; i < 3; ++i)
        if (!isfinite(current[i])) return refuse("non-finite current");
    for (int i = 0; i < 3; ++i) u[i] = (float)(current[i] + 0.0);              // (-0 + 0 = +0: a zero current is +0)
    for (int j = 0; j < waves; ++j) {
        const hydro_sea_wave_t& w = wave[j];
        if (!isfinite(w.amplitude) || !isfinite(w.kx) || !isfinite(w.ky) || !isfinite(w.omega) || !isfinite(w.phase))
            return refuse("non-finite wave component");
        if (w.amplitude < 0.0) return refuse("negative amplitude");
        const double kappa = sqrt(w.kx * w.kx + w.ky * w.ky);
        if (!(kappa > 0.0)) {
            if (w.amplitude != 0.0) return refuse("a wave component with amplitude needs a wave vector (kappa > 0)");
            continue;                                                          // a = 0, kappa = 0: all zeros, contributes +0
        }
        SeaWave& d = out[j];
        const double aw = w.amplitude * w.omega;
        d.omega = w.omega; d.phi = w.phase;
        d.a = (float)w.amplitude; d.kx = (float)w.kx; d.ky = (float)w.ky;
        d.kl2 = (float)(kappa * 1.4426950408889634);
        d.cx = (float)(aw * w.kx / kappa); d.cy = (float)(aw * w.ky / kappa); d.aw = (float)aw;
        if (!isfinite(d.kl2) || !isfinite(d.cx) || !isfinite(d.cy) || !isfinite(d.aw) || !isfinite(d.kx) || !isfinite(d.ky) || !isfinite(d.a))
            return refuse("wave component out of fp32 range");
    }
    return HYDRO_OK;
}

// What hydro_set_sea_finite_depth adds to the records sea_records formed: cx, cy and aw over again from the caller's fp64 values,
// times 1 / (1 - q_j), q_j = e^{-2 kappa_j h}, rounded once; gl_j = -2 kappa_j h log2(e) into `pad`.  (q_j = 0: the deep constants.)
int depth_records(hydro_t* h, const char* what, double depth, int waves, const hydro_sea_wave_t* wave, SeaWave* out)
{
    char msg[128];
    for (int j = 0; j < waves; ++j) {
        const hydro_sea_wave_t& w = wave[j];
        const double kappa = sqrt(w.kx * w.kx + w.ky * w.ky);
        if (!(kappa > 0.0)) continue;                                          // a = 0, kappa = 0: all zeros, contributes +0
        SeaWave& d = out[j];
        const double aw = w.amplitude * w.omega, scale = 1.0 / (1.0 - exp(-2.0 * kappa * depth));
        d.cx = (float)(aw * w.kx / kappa * scale); d.cy = (float)(aw * w.ky / kappa * scale); d.aw = (float)(aw * scale);
        d.pad = (float)(-2.0 * kappa * depth * 1.4426950408889634);
        if (!isfinite(d.cx) || !isfinite(d.cy) || !isfinite(d.aw) || !isfinite(d.pad)) {
            snprintf(msg, sizeof msg, "%s: wave component out of fp32 range at this depth", what);
            return fail(h, HYDRO_E_ARG, msg);
        }
    }
    return HYDRO_OK;
}
}  // namespace

extern "C" {

int hydro_set_sea(hydro_t* h, const hydro_sea_t* sea)
{
    if (!h) return HYDRO_E_ARG;
    if (!sea) { h->sea_waves = -1; return HYDRO_OK; }
    if (h->spectrum_waves >= 0) return fail(h, HYDRO_E_STATE, "a sea spectrum is set (clear it first: hydro_set_sea_spectrum(h, NULL))");
    if (h->ensemble_waves >= 0) return fail(h, HYDRO_E_STATE, "a sea ensemble is set (clear it first: hydro_set_sea_ensemble(h, NULL, 0, 0))");
    if (h->fd_waves >= 0) return fail(h, HYDRO_E_STATE, "a finite-depth sea is set (clear it first: hydro_set_sea_finite_depth(h, NULL, 0, 0, 0))");
    if (sea->waves < 0 || sea->waves > HYDRO_SEA_WAVES_MAX) return fail(h, HYDRO_E_ARG, "sea: waves out of range (0 .. HYDRO_SEA_WAVES_MAX)");
    SeaTable tab;
    memset(&tab, 0, sizeof tab);
    int rc;
    if ((rc = sea_records(h, "sea", sea->current, sea->waves, sea->wave, tab.u, tab.w))) return rc;
    tab.waves = (uint32_t)sea->waves;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (!h->sea_table && hipMalloc(&h->sea_table, sizeof(SeaTable)) != hipSuccess) { h->sea_table = nullptr; return fail(h, HYDRO_E_ALLOC, "sea table: allocation failed"); }
    // from here on the device table is being rewritten: a failure leaves NO sea, never half of one
    h->sea_waves = -1;
    hipError_t e = hipMemcpyAsync(h->sea_table, &tab, sizeof tab, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, HYDRO_E_LAUNCH, "sea table: copy to the device", e);
    h->sea_waves = sea->waves;
    return HYDRO_OK;
}

int hydro_set_sea_spectrum(hydro_t* h, const hydro_sea_spectrum_t* spec)
{
    if (!h) return HYDRO_E_ARG;
    if (!spec) { h->spectrum_waves = -1; return HYDRO_OK; }
    if (h->sea_waves >= 0) return fail(h, HYDRO_E_STATE, "a sea is set (clear it first: hydro_set_sea(h, NULL))");
    if (h->ensemble_waves >= 0) return fail(h, HYDRO_E_STATE, "a sea ensemble is set (clear it first: hydro_set_sea_ensemble(h, NULL, 0, 0))");
    if (h->fd_waves >= 0) return fail(h, HYDRO_E_STATE, "a finite-depth sea is set (clear it first: hydro_set_sea_finite_depth(h, NULL, 0, 0, 0))");
    if (spec->waves < 0 || spec->waves > HYDRO_SPECTRUM_WAVES_MAX)
        return fail(h, HYDRO_E_ARG, "sea spectrum: waves out of range (0 .. HYDRO_SPECTRUM_WAVES_MAX)");
    if (spec->waves > 0 && !spec->wave) return fail(h, HYDRO_E_ARG, "sea spectrum: null wave with waves > 0");
    // (3 KB: on the heap, like the watch tables)
    SpectrumTable* tab = static_cast<SpectrumTable*>(calloc(1, sizeof(SpectrumTable)));
    if (!tab) return fail(h, HYDRO_E_ALLOC, "sea spectrum table: host allocation failed");
    int rc = sea_records(h, "sea spectrum", spec->current, spec->waves, spec->wave, tab->u, tab->w);
    if (rc) { free(tab); return rc; }
    tab->waves = (uint32_t)spec->waves;
    if (const hipError_t e = use_device(h->device); e != hipSuccess) { free(tab); return fail(h, HYDRO_E_DEVICE, "use_device(h->device)", e); }
    if (!h->spectrum_table && hipMalloc(&h->spectrum_table, sizeof(SpectrumTable)) != hipSuccess) {
        h->spectrum_table = nullptr;
        free(tab);
        return fail(h, HYDRO_E_ALLOC, "sea spectrum table: allocation failed");
    }
    // from here on the device table is being rewritten: a failure leaves NO spectrum, never half of one
    h->spectrum_waves = -1;
    hipError_t e = hipMemcpyAsync(h->spectrum_table, tab, sizeof *tab, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    free(tab);
    if (e != hipSuccess) return fail(h, HYDRO_E_LAUNCH, "sea spectrum table: copy to the device", e);
    h->spectrum_waves = spec->waves;
    return HYDRO_OK;
}

int hydro_set_sea_ensemble(hydro_t* h, const hydro_sea_spectrum_t* members, int64_t count, int64_t bodies_per_sea)
{
    if (!h) return HYDRO_E_ARG;
    if (!members) { h->ensemble_waves = -1; return HYDRO_OK; }
    if (h->sea_waves >= 0) return fail(h, HYDRO_E_STATE, "a sea is set (clear it first: hydro_set_sea(h, NULL))");
    if (h->spectrum_waves >= 0) return fail(h, HYDRO_E_STATE, "a sea spectrum is set (clear it first: hydro_set_sea_spectrum(h, NULL))");
    if (h->fd_waves >= 0) return fail(h, HYDRO_E_STATE, "a finite-depth sea is set (clear it first: hydro_set_sea_finite_depth(h, NULL, 0, 0, 0))");
    if (count < 1 || count > HYDRO_SEA_ENSEMBLE_MAX) return fail(h, HYDRO_E_ARG, "sea ensemble: count out of range (1 .. HYDRO_SEA_ENSEMBLE_MAX)");
    if (bodies_per_sea < HYDRO_TILE || bodies_per_sea % HYDRO_TILE != 0 || bodies_per_sea >= ((int64_t)1 << 31))
        return fail(h, HYDRO_E_ARG, "sea ensemble: bodies_per_sea must be a positive multiple of 64 (and < 2^31)");
    const int waves = members[0].waves;
    if (waves < 0 || waves > HYDRO_SPECTRUM_WAVES_MAX)
        return fail(h, HYDRO_E_ARG, "sea ensemble: waves out of range (0 .. HYDRO_SPECTRUM_WAVES_MAX)");
    for (int64_t m = 0; m < count; ++m) {
        if (members[m].waves != waves) return fail(h, HYDRO_E_ARG, "sea ensemble: every member must have the same number of waves");
        if (waves > 0 && !members[m].wave) return fail(h, HYDRO_E_ARG, "sea ensemble: null wave with waves > 0");
    }
    // (up to 3 MB: on the heap.  Everything is checked and formed here, before the device table is touched)
    SpectrumTable* tab = static_cast<SpectrumTable*>(calloc((size_t)count, sizeof(SpectrumTable)));
    if (!tab) return fail(h, HYDRO_E_ALLOC, "sea ensemble table: host allocation failed");
    for (int64_t m = 0; m < count; ++m) {
        char what[48];
        snprintf(what, sizeof what, "sea ensemble member %lld", (long long)m);
        const int rc = sea_records(h, what, members[m].current, waves, members[m].wave, tab[m].u, tab[m].w);
        if (rc) { free(tab); return rc; }
        tab[m].waves = (uint32_t)waves;
    }
    if (const hipError_t e = use_device(h->device); e != hipSuccess) { free(tab); return fail(h, HYDRO_E_DEVICE, "use_device(h->device)", e); }
    if (count > h->ensemble_capacity) {
        // a larger table: the new one first, so that a failure leaves the previous ensemble in force
        void* grown = nullptr;
        if (hipMalloc(&grown, (size_t)count * sizeof(SpectrumTable)) != hipSuccess) {
            free(tab);
            return fail(h, HYDRO_E_ALLOC, "sea ensemble table: allocation failed");
        }
        if (h->ensemble_table) (void)hipFree(h->ensemble_table);
        h->ensemble_table = grown;
        h->ensemble_capacity = count;
    }
    // from here on the device table is being rewritten: a failure leaves NO ensemble, never half of one
    h->ensemble_waves = -1;
    hipError_t e = hipMemcpyAsync(h->ensemble_table, tab, (size_t)count * sizeof(SpectrumTable), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    free(tab);
    if (e != hipSuccess) return fail(h, HYDRO_E_LAUNCH, "sea ensemble table: copy to the device", e);
    h->ensemble_count = count;
    h->ensemble_tiles_per_sea = bodies_per_sea / HYDRO_TILE;
    h->ensemble_waves = waves;
    return HYDRO_OK;
}

int hydro_set_sea_finite_depth(hydro_t* h, const hydro_sea_spectrum_t* members, int64_t count, int64_t bodies_per_sea, double depth)
{
    if (!h) return HYDRO_E_ARG;
    if (!members) { h->fd_waves = -1; return HYDRO_OK; }
    if (h->sea_waves >= 0) return fail(h, HYDRO_E_STATE, "a sea is set (clear it first: hydro_set_sea(h, NULL))");
    if (h->spectrum_waves >= 0) return fail(h, HYDRO_E_STATE, "a sea spectrum is set (clear it first: hydro_set_sea_spectrum(h, NULL))");
    if (h->ensemble_waves >= 0) return fail(h, HYDRO_E_STATE, "a sea ensemble is set (clear it first: hydro_set_sea_ensemble(h, NULL, 0, 0))");
    if (count < 1 || count > HYDRO_SEA_ENSEMBLE_MAX) return fail(h, HYDRO_E_ARG, "finite-depth sea: count out of range (1 .. HYDRO_SEA_ENSEMBLE_MAX)");
    if (bodies_per_sea < HYDRO_TILE || bodies_per_sea % HYDRO_TILE != 0 || bodies_per_sea >= ((int64_t)1 << 31))
        return fail(h, HYDRO_E_ARG, "finite-depth sea: bodies_per_sea must be a positive multiple of 64 (and < 2^31)");
    const float neg_depth = (float)-depth;                                     // -h, rounded once
    if (!isfinite(depth) || !(depth > 0.0) || !isfinite(neg_depth) || !(neg_depth < 0.0f))
        return fail(h, HYDRO_E_ARG, "finite-depth sea: depth must be finite and > 0 (and in fp32 range)");
    const int waves = members[0].waves;
    if (waves < 0 || waves > HYDRO_SPECTRUM_WAVES_MAX)
        return fail(h, HYDRO_E_ARG, "finite-depth sea: waves out of range (0 .. HYDRO_SPECTRUM_WAVES_MAX)");
    for (int64_t m = 0; m < count; ++m) {
        if (members[m].waves != waves) return fail(h, HYDRO_E_ARG, "finite-depth sea: every member must have the same number of waves");
        if (waves > 0 && !members[m].wave) return fail(h, HYDRO_E_ARG, "finite-depth sea: null wave with waves > 0");
    }
    // (everything is checked and formed on the host, before the device table is touched)
    SpectrumTable* tab = static_cast<SpectrumTable*>(calloc((size_t)count, sizeof(SpectrumTable)));
    if (!tab) return fail(h, HYDRO_E_ALLOC, "finite-depth sea table: host allocation failed");
    for (int64_t m = 0; m < count; ++m) {
        char what[48];
        snprintf(what, sizeof what, "finite-depth sea member %lld", (long long)m);
        int rc = sea_records(h, what, members[m].current, waves, members[m].wave, tab[m].u, tab[m].w);
        if (!rc) rc = depth_records(h, what, depth, waves, members[m].wave, tab[m].w);
        if (rc) { free(tab); return rc; }
        tab[m].waves = (uint32_t)waves;
    }
    if (const hipError_t e = use_device(h->device); e != hipSuccess) { free(tab); return fail(h, HYDRO_E_DEVICE, "use_device(h->device)", e); }
    if (count > h->fd_capacity) {
        // a larger table: the new one first, so that a failure leaves the previous sea in force
        void* grown = nullptr;
        if (hipMalloc(&grown, (size_t)count * sizeof(SpectrumTable)) != hipSuccess) {
            free(tab);
            return fail(h, HYDRO_E_ALLOC, "finite-depth sea table: allocation failed");
        }
        if (h->fd_table) (void)hipFree(h->fd_table);
        h->fd_table = grown;
        h->fd_capacity = count;
    }
    // from here on the device table is being rewritten: a failure leaves NO finite-depth sea, never half of one
    h->fd_waves = -1;
    hipError_t e = hipMemcpyAsync(h->fd_table, tab, (size_t)count * sizeof(SpectrumTable), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    free(tab);
    if (e != hipSuccess) return fail(h, HYDRO_E_LAUNCH, "finite-depth sea table: copy to the device", e);
    h->fd_count = count;
    h->fd_tiles_per_sea = bodies_per_sea / HYDRO_TILE;
    h->fd_neg_depth = neg_depth;
    h->fd_waves = waves;
    return HYDRO_OK;
}

int hydro_set_current_profile(hydro_t* h, const hydro_current_profile_t* profile)
{
    if (!h) return HYDRO_E_ARG;
    if (!profile || profile->knots == 0) { h->shear_knots = 0; return HYDRO_OK; }
    const int knots = profile->knots;
    if (knots < 0 || knots > HYDRO_CURRENT_KNOTS_MAX) return fail(h, HYDRO_E_ARG, "current profile: knots out of range (0 .. HYDRO_CURRENT_KNOTS_MAX)");
    if (!profile->z || !profile->v) return fail(h, HYDRO_E_ARG, "current profile: null z or v with knots > 0");
    // (everything is checked and formed on the host, before the device table is touched)
    CurrentTable tab;
    memset(&tab, 0, sizeof tab);
    for (int l = 0; l < knots; ++l) {
        const float z = profile->z[l], *v = profile->v + 3 * l;
        if (!isfinite(z) || !isfinite(v[0]) || !isfinite(v[1]) || !isfinite(v[2])) return fail(h, HYDRO_E_ARG, "current profile: non-finite knot");
        if (z > 0.0f) return fail(h, HYDRO_E_ARG, "current profile: a knot above the still-water surface (z > 0)");
        if (l > 0 && !(z > profile->z[l - 1])) return fail(h, HYDRO_E_ARG, "current profile: z must be strictly ascending (in fp32)");
    }
    tab.v0[0] = profile->v[0]; tab.v0[1] = profile->v[1]; tab.v0[2] = profile->v[2];
    tab.knots = (uint32_t)knots;
    for (int l = 0; l + 1 < knots; ++l) {
        CurrentKnot& k = tab.k[l];
        k.z = profile->z[l];
        k.inv = (float)(1.0 / ((double)profile->z[l + 1] - (double)profile->z[l]));
        for (int i = 0; i < 3; ++i) k.d[i] = (float)((double)profile->v[3 * (l + 1) + i] - (double)profile->v[3 * l + i]);
        if (!isfinite(k.inv) || !isfinite(k.d[0]) || !isfinite(k.d[1]) || !isfinite(k.d[2]))
            return fail(h, HYDRO_E_ARG, "current profile: a segment's 1 / (z_{l+1} - z_l) or V_{l+1} - V_l is out of fp32 range");
    }
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (!h->shear_table) HYDRO_HIP(h, hipMalloc(&h->shear_table, sizeof(CurrentTable)), HYDRO_E_ALLOC);
    // from here on the device table is being rewritten: a failure leaves NO profile, never half of one
    h->shear_knots = 0;
    HYDRO_HIP(h, hipMemcpyAsync(h->shear_table, &tab, sizeof tab, hipMemcpyHostToDevice, h->stream), HYDRO_E_LAUNCH);
    HYDRO_HIP(h, hipStreamSynchronize(h->stream), HYDRO_E_LAUNCH);
    h->shear_knots = knots;
    return HYDRO_OK;
}

}  // extern "C"

namespace {
// hydro_sea_sample, hydro_sea_spectrum_sample and hydro_sea_ensemble_sample: one set of rules, the table and the kernel of each;
// `members` (the ensemble's and the finite-depth sea's only: the others pass none) are count and tiles_per_sea - a refusal of its own,
// last, and the kernel's next argument - and then whatever else the kernel takes (the finite-depth sea's -h).
template <typename Kernel, typename... Members>
int water_sample(hydro_t* h, Kernel kernel, const void* table, int waves, const char* none, int64_t n, const float* state, int64_t state_tile_stride,
                 int64_t step_index, double dt, float* out, int64_t out_tile_stride, void* stream, Members... members)
{
    if (!h) return HYDRO_E_ARG;
    if (n < 0 || n > h->capacity) return fail(h, HYDRO_E_ARG, "n out of range (0 <= n <= capacity)");
    if (waves < 0) return fail(h, HYDRO_E_STATE, none);
    if (!(dt > 0.0)) return fail(h, HYDRO_E_ARG, "dt must be > 0");
    if (step_index < 0 || step_index >= ((int64_t)1 << 52)) return fail(h, HYDRO_E_ARG, "step_index must be in 0 .. 2^52 - 1");
    int rc;
    if ((rc = check_tiled(h, n, state, state_tile_stride, HYDRO_STATE_FIELDS, "null state"))) return rc;
    if ((rc = check_tiled(h, n, out, out_tile_stride, HYDRO_SEA_FIELDS, "null out"))) return rc;
    if constexpr (sizeof...(Members) != 0) {
        const bool covered = [&](int64_t count, int64_t tiles_per_sea, auto...) {
            return ((n + HYDRO_TILE - 1) / HYDRO_TILE + tiles_per_sea - 1) / tiles_per_sea <= count;
        }(members...);
        if (!covered)
            return fail(h, HYDRO_E_ARG, sizeof...(Members) > 2 ? "n needs more members than the finite-depth sea has (count * bodies_per_sea < n)"
                                                               : "n needs more members than the sea ensemble has (count * bodies_per_sea < n)");
    }
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (n == 0) return HYDRO_OK;
    const auto launch = [&](auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), state, (uint32_t)state_tile_stride,
                           out, (uint32_t)out_tile_stride, (uint32_t)n, table, (uint32_t)waves, step_index, dt, tail...);
    };
    if constexpr (sizeof...(Members) != 0)
        [&](int64_t, int64_t tiles_per_sea, auto... more) { launch((uint32_t)tiles_per_sea, more...); }(members...);
    else launch();
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}
}  // namespace

extern "C" {

int hydro_sea_sample(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride, int64_t step_index, double dt,
                     float* out, int64_t out_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    return water_sample(h, sea_sample_kernel, (const void*)h->sea_table, h->sea_waves, "no sea (call hydro_set_sea first)",
                        n, state, state_tile_stride, step_index, dt, out, out_tile_stride, stream);
}

int hydro_sea_spectrum_sample(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride, int64_t step_index, double dt,
                              float* out, int64_t out_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    return water_sample(h, spectrum_sample_kernel, (const void*)h->spectrum_table, h->spectrum_waves, "no sea spectrum (call hydro_set_sea_spectrum first)",
                        n, state, state_tile_stride, step_index, dt, out, out_tile_stride, stream);
}

int hydro_sea_ensemble_sample(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride, int64_t step_index, double dt,
                              float* out, int64_t out_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    return water_sample(h, ensemble_sample_kernel, (const void*)h->ensemble_table, h->ensemble_waves, "no sea ensemble (call hydro_set_sea_ensemble first)",
                        n, state, state_tile_stride, step_index, dt, out, out_tile_stride, stream, h->ensemble_count, h->ensemble_tiles_per_sea);
}

int hydro_sea_finite_depth_sample(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride, int64_t step_index, double dt,
                                  float* out, int64_t out_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    return water_sample(h, depth_sample_kernel, (const void*)h->fd_table, h->fd_waves, "no finite-depth sea (call hydro_set_sea_finite_depth first)",
                        n, state, state_tile_stride, step_index, dt, out, out_tile_stride, stream, h->fd_count, h->fd_tiles_per_sea, h->fd_neg_depth);
}

int hydro_current_profile_sample(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride, int64_t step_index, double dt,
                                 float* out, int64_t out_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    if (h->shear_knots == 0)                                                   // no profile: the _fd sample, its launch and its bits
        return hydro_sea_finite_depth_sample(h, n, state, state_tile_stride, step_index, dt, out, out_tile_stride, stream);
    return water_sample(h, shear_sample_kernel, (const void*)h->fd_table, h->fd_waves, "no finite-depth sea (call hydro_set_sea_finite_depth first)",
                        n, state, state_tile_stride, step_index, dt, out, out_tile_stride, stream, h->fd_count, h->fd_tiles_per_sea, h->fd_neg_depth,
                        (const void*)h->shear_table, (uint32_t)h->shear_knots);
}

int hydro_step_fused_tiled_multi_sea(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                     const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                     float* state_out, int64_t out_tile_stride,
                                     float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double* ke_out_dev,
                                     float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t* rows_written_host,
                                     const float* applied, int64_t applied_tile_stride, int applied_frame,
                                     const float* control, int64_t control_tile_stride, int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_set_seabed(hydro_t* h, const hydro_seabed_t* bed)
{
    if (!h) return HYDRO_E_ARG;
    if (!bed) { h->has_bed = false; return HYDRO_OK; }
    const double v[6] = {bed->z, bed->stiffness, bed->damping, bed->friction, bed->slip_speed, bed->friction_rate};
    for (int i = 0; i < 6; ++i)
        if (!isfinite(v[i])) return fail(h, HYDRO_E_ARG, "seabed: non-finite value");
    if (bed->stiffness < 0.0 || bed->damping < 0.0 || bed->friction < 0.0 || bed->friction_rate < 0.0)
        return fail(h, HYDRO_E_ARG, "seabed: stiffness, damping, friction and friction_rate must be >= 0");
    if (!(bed->slip_speed > 0.0)) return fail(h, HYDRO_E_ARG, "seabed: slip_speed must be > 0");
    // rounded ONCE; the slip speed must stay positive in fp32, and its square too (it is what keeps the friction's 1/sqrt finite)
    const Seabed b = {(float)(bed->z + 0.0), (float)(bed->stiffness + 0.0), (float)(bed->damping + 0.0), (float)(bed->friction + 0.0),
                      (float)bed->slip_speed, (float)(bed->friction_rate + 0.0)};
    if (!isfinite(b.z) || !isfinite(b.stiffness) || !isfinite(b.damping) || !isfinite(b.friction) || !isfinite(b.slip_speed)
        || !isfinite(b.friction_rate) || !(b.slip_speed * b.slip_speed > 0.0f) || !isfinite(b.slip_speed * b.slip_speed))
        return fail(h, HYDRO_E_ARG, "seabed: constant out of fp32 range");
    h->bed = b;
    h->has_bed = true;
    return HYDRO_OK;
}

int hydro_seabed_wrench(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride, float* out, int64_t out_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    if (!h->has_bed) return fail(h, HYDRO_E_STATE, "no seabed (call hydro_set_seabed first)");
    int rc;
    if ((rc = check_common(h, n))) return rc;
    if ((rc = check_tiled(h, n, state, state_tile_stride, HYDRO_STATE_FIELDS, "null state"))) return rc;
    if ((rc = check_tiled(h, n, out, out_tile_stride, HYDRO_WRENCH_FIELDS, "null out"))) return rc;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (n == 0) return HYDRO_OK;
    hipLaunchKernelGGL(seabed_wrench_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), state, (uint32_t)state_tile_stride,
                       (const float*)h->params_tiled, prm_tile_floats(h), prm_mass_field(h), out, (uint32_t)out_tile_stride, (uint32_t)n, h->bed);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int hydro_step_fused_tiled_multi_bed(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                     const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                     float* state_out, int64_t out_tile_stride,
                                     float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double* ke_out_dev,
                                     float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t* rows_written_host,
                                     const float* applied, int64_t applied_tile_stride, int applied_frame,
                                     const float* control, int64_t control_tile_stride, int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_mooring_wrench(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride, const float* mooring, int64_t mooring_tile_stride,
                         float* out, int64_t out_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    int rc;
    if ((rc = check_common(h, n))) return rc;
    if ((rc = check_tiled(h, n, state, state_tile_stride, HYDRO_STATE_FIELDS, "null state"))) return rc;
    if ((rc = check_tiled(h, n, mooring, mooring_tile_stride, HYDRO_MOOR_FIELDS, "null mooring"))) return rc;
    if ((rc = check_tiled(h, n, out, out_tile_stride, HYDRO_WRENCH_FIELDS, "null out"))) return rc;
    const int64_t tiles = (n + HYDRO_TILE - 1) / HYDRO_TILE, out_floats = tiled_extent(tiles, out_tile_stride, HYDRO_WRENCH_FIELDS);
    if (ranges_overlap(state, tiled_extent(tiles, state_tile_stride, HYDRO_STATE_FIELDS), out, out_floats)
        || ranges_overlap(mooring, tiled_extent(tiles, mooring_tile_stride, HYDRO_MOOR_FIELDS), out, out_floats))
        return fail(h, HYDRO_E_ARG, "out must not overlap an input (state, mooring)");
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (n == 0) return HYDRO_OK;
    hipLaunchKernelGGL(mooring_wrench_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), state, (uint32_t)state_tile_stride,
                       mooring, (uint32_t)mooring_tile_stride, out, (uint32_t)out_tile_stride, (uint32_t)n);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int hydro_step_fused_tiled_multi_moor(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                      const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                      float* state_out, int64_t out_tile_stride,
                                      float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                      int rotational, double* ke_out_dev,
                                      float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                      int64_t row0, int64_t* rows_written_host,
                                      const float* applied, int64_t applied_tile_stride, int applied_frame,
                                      const float* control, int64_t control_tile_stride,
                                      const float* mooring, int64_t mooring_tile_stride, int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_extremes_reset(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                         float* extremes, int64_t extremes_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    int rc;
    if (n < 0 || n > h->capacity) return fail(h, HYDRO_E_ARG, "n out of range (0 .. capacity)");
    if (state && (rc = check_tiled(h, n, state, state_tile_stride, HYDRO_STATE_FIELDS, "null state"))) return rc;
    if ((rc = check_tiled(h, n, extremes, extremes_tile_stride, HYDRO_EXT_FIELDS, "null extremes"))) return rc;
    const int64_t tiles = (n + HYDRO_TILE - 1) / HYDRO_TILE;
    if (state && ranges_overlap(state, tiled_extent(tiles, state_tile_stride, HYDRO_STATE_FIELDS), extremes, tiled_extent(tiles, extremes_tile_stride, HYDRO_EXT_FIELDS)))
        return fail(h, HYDRO_E_ARG, "extremes must not overlap state");
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (n == 0) return HYDRO_OK;
    hipLaunchKernelGGL(extremes_reset_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       state, state ? (uint32_t)state_tile_stride : 0u, extremes, (uint32_t)extremes_tile_stride, (uint32_t)n);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int hydro_step_fused_tiled_multi_ext(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                     const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                     float* state_out, int64_t out_tile_stride,
                                     float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double* ke_out_dev,
                                     float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t* rows_written_host,
                                     const float* applied, int64_t applied_tile_stride, int applied_frame,
                                     const float* control, int64_t control_tile_stride,
                                     const float* mooring, int64_t mooring_tile_stride,
                                     float* extremes, int64_t extremes_tile_stride, int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    m.with_extremes(extremes, extremes_tile_stride);
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_tether_wrench(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride, const float* tether, int64_t tether_tile_stride,
                        float* out, int64_t out_tile_stride, float* tension, int64_t tension_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    int rc;
    if ((rc = check_common(h, n))) return rc;
    if ((rc = check_tiled(h, n, state, state_tile_stride, HYDRO_STATE_FIELDS, "null state"))) return rc;
    if ((rc = check_tiled(h, n, tether, tether_tile_stride, HYDRO_TETH_FIELDS, "null tether"))) return rc;
    if ((rc = check_tiled(h, n, out, out_tile_stride, HYDRO_WRENCH_FIELDS, "null out"))) return rc;
    if (tension && (rc = check_tiled(h, n, tension, tension_tile_stride, 1, "null tension"))) return rc;
    const int64_t tiles = (n + HYDRO_TILE - 1) / HYDRO_TILE, out_floats = tiled_extent(tiles, out_tile_stride, HYDRO_WRENCH_FIELDS);
    const int64_t state_floats = tiled_extent(tiles, state_tile_stride, HYDRO_STATE_FIELDS), tether_floats = tiled_extent(tiles, tether_tile_stride, HYDRO_TETH_FIELDS);
    if (ranges_overlap(state, state_floats, out, out_floats) || ranges_overlap(tether, tether_floats, out, out_floats))
        return fail(h, HYDRO_E_ARG, "out must not overlap an input (state, tether)");
    if (tension) {
        const int64_t tension_floats = tiled_extent(tiles, tension_tile_stride, 1);
        if (ranges_overlap(state, state_floats, tension, tension_floats) || ranges_overlap(tether, tether_floats, tension, tension_floats)
            || ranges_overlap(out, out_floats, tension, tension_floats))
            return fail(h, HYDRO_E_ARG, "tension must not overlap an input (state, tether) or out");
    }
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (n == 0) return HYDRO_OK;
    hipLaunchKernelGGL(tether_wrench_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), state, (uint32_t)state_tile_stride,
                       tether, (uint32_t)tether_tile_stride, out, (uint32_t)out_tile_stride, tension, tension ? (uint32_t)tension_tile_stride : 0u, (uint32_t)n);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int hydro_step_fused_tiled_multi_teth(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                      const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                      float* state_out, int64_t out_tile_stride,
                                      float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                      int rotational, double* ke_out_dev,
                                      float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                      int64_t row0, int64_t* rows_written_host,
                                      const float* applied, int64_t applied_tile_stride, int applied_frame,
                                      const float* control, int64_t control_tile_stride,
                                      const float* mooring, int64_t mooring_tile_stride,
                                      float* extremes, int64_t extremes_tile_stride,
                                      const float* tether, int64_t tether_tile_stride, int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    m.with_extremes(extremes, extremes_tile_stride);
    m.with_tether(tether, tether_tile_stride);
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_step_fused_tiled_multi_net(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                     const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                     float* state_out, int64_t out_tile_stride,
                                     float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double* ke_out_dev,
                                     float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t* rows_written_host,
                                     const float* applied, int64_t applied_tile_stride, int applied_frame,
                                     const float* control, int64_t control_tile_stride,
                                     const float* mooring, int64_t mooring_tile_stride,
                                     float* extremes, int64_t extremes_tile_stride,
                                     const float* tether, int64_t tether_tile_stride, int64_t tether_layers, int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    m.with_extremes(extremes, extremes_tile_stride);
    m.with_tether(tether, tether_tile_stride);
    m.with_layers(tether_layers);
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_step_fused_tiled_multi_peak(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                      const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                      float* state_out, int64_t out_tile_stride,
                                      float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                      int rotational, double* ke_out_dev,
                                      float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                      int64_t row0, int64_t* rows_written_host,
                                      const float* applied, int64_t applied_tile_stride, int applied_frame,
                                      const float* control, int64_t control_tile_stride,
                                      const float* mooring, int64_t mooring_tile_stride,
                                      float* extremes, int64_t extremes_tile_stride,
                                      const float* tether, int64_t tether_tile_stride, int64_t tether_layers,
                                      float* tether_peaks, int64_t tether_peaks_tile_stride, int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    m.with_extremes(extremes, extremes_tile_stride);
    m.with_tether(tether, tether_tile_stride);
    m.with_layers(tether_layers);
    m.with_peaks(tether_peaks, tether_peaks_tile_stride);
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_step_fused_tiled_multi_spread(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                        const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                        float* state_out, int64_t out_tile_stride,
                                        float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                        int rotational, double* ke_out_dev,
                                        float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                        int64_t row0, int64_t* rows_written_host,
                                        const float* applied, int64_t applied_tile_stride, int applied_frame,
                                        const float* control, int64_t control_tile_stride,
                                        const float* mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                        float* extremes, int64_t extremes_tile_stride,
                                        const float* tether, int64_t tether_tile_stride, int64_t tether_layers,
                                        float* tether_peaks, int64_t tether_peaks_tile_stride, int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    m.with_mooring_layers(mooring_layers);
    m.with_extremes(extremes, extremes_tile_stride);
    m.with_tether(tether, tether_tile_stride);
    m.with_layers(tether_layers);
    m.with_peaks(tether_peaks, tether_peaks_tile_stride);
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_step_fused_tiled_multi_irr(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                     const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                     float* state_out, int64_t out_tile_stride,
                                     float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double* ke_out_dev,
                                     float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t* rows_written_host,
                                     const float* applied, int64_t applied_tile_stride, int applied_frame,
                                     const float* control, int64_t control_tile_stride,
                                     const float* mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                     float* extremes, int64_t extremes_tile_stride,
                                     const float* tether, int64_t tether_tile_stride, int64_t tether_layers,
                                     float* tether_peaks, int64_t tether_peaks_tile_stride, int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    m.with_mooring_layers(mooring_layers);
    m.with_extremes(extremes, extremes_tile_stride);
    m.with_tether(tether, tether_tile_stride);
    m.with_layers(tether_layers);
    m.with_peaks(tether_peaks, tether_peaks_tile_stride);
    m.with_spectrum();
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_statistics_reset(hydro_t* h, int64_t n, void* statistics, int64_t statistics_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    int rc;
    if (n < 0 || n > h->capacity) return fail(h, HYDRO_E_ARG, "n out of range (0 .. capacity)");
    if ((rc = check_tiled(h, n, statistics, statistics_tile_stride, HYDRO_STAT_BYTES_PER_BODY / 4, "null statistics"))) return rc;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    if (n == 0) return HYDRO_OK;
    hipLaunchKernelGGL(statistics_reset_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       statistics, (uint32_t)statistics_tile_stride, (uint32_t)n);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int hydro_step_fused_tiled_multi_stat(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                      const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                      float* state_out, int64_t out_tile_stride,
                                      float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                      int rotational, double* ke_out_dev,
                                      float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                      int64_t row0, int64_t* rows_written_host,
                                      const float* applied, int64_t applied_tile_stride, int applied_frame,
                                      const float* control, int64_t control_tile_stride,
                                      const float* mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                      float* extremes, int64_t extremes_tile_stride,
                                      const float* tether, int64_t tether_tile_stride, int64_t tether_layers,
                                      float* tether_peaks, int64_t tether_peaks_tile_stride,
                                      void* statistics, int64_t statistics_tile_stride,
                                      const float* levels, int64_t levels_tile_stride, int channel_a, int channel_b,
                                      int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    m.with_mooring_layers(mooring_layers);
    m.with_extremes(extremes, extremes_tile_stride);
    m.with_tether(tether, tether_tile_stride);
    m.with_layers(tether_layers);
    m.with_peaks(tether_peaks, tether_peaks_tile_stride);
    m.with_spectrum();
    m.with_statistics(statistics, statistics_tile_stride, levels, levels_tile_stride, channel_a, channel_b);
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_step_fused_tiled_multi_ens(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                     const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                     float* state_out, int64_t out_tile_stride,
                                     float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                     int rotational, double* ke_out_dev,
                                     float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                     int64_t row0, int64_t* rows_written_host,
                                     const float* applied, int64_t applied_tile_stride, int applied_frame,
                                     const float* control, int64_t control_tile_stride,
                                     const float* mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                     float* extremes, int64_t extremes_tile_stride,
                                     const float* tether, int64_t tether_tile_stride, int64_t tether_layers,
                                     float* tether_peaks, int64_t tether_peaks_tile_stride,
                                     void* statistics, int64_t statistics_tile_stride,
                                     const float* levels, int64_t levels_tile_stride, int channel_a, int channel_b,
                                     int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    m.with_mooring_layers(mooring_layers);
    m.with_extremes(extremes, extremes_tile_stride);
    m.with_tether(tether, tether_tile_stride);
    m.with_layers(tether_layers);
    m.with_peaks(tether_peaks, tether_peaks_tile_stride);
    m.with_spectrum();
    m.with_statistics(statistics, statistics_tile_stride, levels, levels_tile_stride, channel_a, channel_b);
    m.with_ensemble();
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_step_fused_tiled_multi_fd(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                    const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                    float* state_out, int64_t out_tile_stride,
                                    float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                    int rotational, double* ke_out_dev,
                                    float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                    int64_t row0, int64_t* rows_written_host,
                                    const float* applied, int64_t applied_tile_stride, int applied_frame,
                                    const float* control, int64_t control_tile_stride,
                                    const float* mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                    float* extremes, int64_t extremes_tile_stride,
                                    const float* tether, int64_t tether_tile_stride, int64_t tether_layers,
                                    float* tether_peaks, int64_t tether_peaks_tile_stride,
                                    void* statistics, int64_t statistics_tile_stride,
                                    const float* levels, int64_t levels_tile_stride, int channel_a, int channel_b,
                                    int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    m.with_mooring_layers(mooring_layers);
    m.with_extremes(extremes, extremes_tile_stride);
    m.with_tether(tether, tether_tile_stride);
    m.with_layers(tether_layers);
    m.with_peaks(tether_peaks, tether_peaks_tile_stride);
    m.with_spectrum();
    m.with_statistics(statistics, statistics_tile_stride, levels, levels_tile_stride, channel_a, channel_b);
    m.with_ensemble();
    m.with_finite_depth();
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_step_fused_tiled_multi_shear(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride,
                                       const float* prev, int64_t prev_tile_stride, double dt, int steps,
                                       float* state_out, int64_t out_tile_stride,
                                       float* prev_out, int64_t prev_out_tile_stride, int implicit_drag,
                                       int rotational, double* ke_out_dev,
                                       float* log, int64_t log_stride, int64_t rows_capacity, int fields, int every, int phase,
                                       int64_t row0, int64_t* rows_written_host,
                                       const float* applied, int64_t applied_tile_stride, int applied_frame,
                                       const float* control, int64_t control_tile_stride,
                                       const float* mooring, int64_t mooring_tile_stride, int64_t mooring_layers,
                                       float* extremes, int64_t extremes_tile_stride,
                                       const float* tether, int64_t tether_tile_stride, int64_t tether_layers,
                                       float* tether_peaks, int64_t tether_peaks_tile_stride,
                                       void* statistics, int64_t statistics_tile_stride,
                                       const float* levels, int64_t levels_tile_stride, int channel_a, int channel_b,
                                       int64_t step0, void* stream)
{
    MultiStep m = {n, state, state_tile_stride, prev, prev_tile_stride, dt, steps, state_out, out_tile_stride, prev_out, prev_out_tile_stride,
                   implicit_drag, rotational, ke_out_dev, stream};
    m.with_recorder(log, log_stride, rows_capacity, fields, every, phase, row0, rows_written_host);
    m.with_applied(applied, applied_tile_stride, applied_frame);
    m.with_control(control, control_tile_stride);
    m.with_sea(step0);
    m.with_seabed();
    m.with_mooring(mooring, mooring_tile_stride);
    m.with_mooring_layers(mooring_layers);
    m.with_extremes(extremes, extremes_tile_stride);
    m.with_tether(tether, tether_tile_stride);
    m.with_layers(tether_layers);
    m.with_peaks(tether_peaks, tether_peaks_tile_stride);
    m.with_spectrum();
    m.with_statistics(statistics, statistics_tile_stride, levels, levels_tile_stride, channel_a, channel_b);
    m.with_ensemble();
    m.with_finite_depth();
    m.with_current_profile();
    return step_fused_tiled_multi_launch(h, m);
}

int hydro_pack_state_aos(hydro_t* h, int64_t n, const float* positions, const float* orientations, int quat_xyzw,
                         const float* velocities, float* state, int64_t state_tile_stride, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    if (n < 0 || n > h->capacity) return fail(h, HYDRO_E_ARG, "n out of range (0 <= n <= capacity)");
    if (!positions || !orientations || !velocities) return fail(h, HYDRO_E_ARG, "null tensor pointer");
    if (!aligned_to(positions, 16) || !aligned_to(orientations, 16) || !aligned_to(velocities, 16))
        return fail(h, HYDRO_E_ARG, "array-of-structs tensors must be 16-byte aligned");
    int rc = check_tiled(h, n, state, state_tile_stride, HYDRO_STATE_FIELDS, "null state");
    if (rc) return rc;
    if (n == 0) return HYDRO_OK;
    PackArgs a;
    a.pos = positions; a.quat = orientations; a.vel = velocities; a.quat_xyzw = quat_xyzw ? 1 : 0;
    a.st = state; a.st_stride = (uint32_t)state_tile_stride; a.n = (uint32_t)n;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipLaunchKernelGGL(pack_state_aos_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int hydro_unpack_wrench_aos(hydro_t* h, int64_t n, const float* wrench, int64_t wrench_tile_stride,
                            float* forces, float* torques, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    if (n < 0 || n > h->capacity) return fail(h, HYDRO_E_ARG, "n out of range (0 <= n <= capacity)");
    if (!forces || !torques) return fail(h, HYDRO_E_ARG, "null tensor pointer");
    if (!aligned_to(forces, 16) || !aligned_to(torques, 16)) return fail(h, HYDRO_E_ARG, "array-of-structs tensors must be 16-byte aligned");
    int rc = check_tiled(h, n, wrench, wrench_tile_stride, HYDRO_WRENCH_FIELDS, "null wrench");
    if (rc) return rc;
    if (n == 0) return HYDRO_OK;
    UnpackArgs a;
    a.w = wrench; a.w_stride = (uint32_t)wrench_tile_stride; a.force = forces; a.torque = torques; a.n = (uint32_t)n;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipLaunchKernelGGL(unpack_wrench_aos_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int hydro_repack(hydro_t* h, int64_t n, int fields, float* const soa[], float* tiled, int64_t tile_stride,
                 int to_tiled, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    if (n < 0 || n > h->capacity || !soa || fields < 1 || fields > 24) return fail(h, HYDRO_E_ARG, "bad arguments");
    for (int f = 0; f < fields; ++f) if (!soa[f]) return fail(h, HYDRO_E_ARG, "null field pointer");
    int rc = check_tiled(h, n, tiled, tile_stride, fields, "null tiled buffer");
    if (rc) return rc;
    if (n == 0) return HYDRO_OK;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    return repack(h, soa, fields, tiled, tile_stride, n, to_tiled != 0, static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace {
// hydro_step_wrench_aos; sea_time: the _sea entry - the time is checked first, and the step goes through the sea if one is set;
// irr_entry: the _irr entry - the _sea entry, and a spectrum, an ensemble or a finite-depth sea counts as well
int step_wrench_aos_impl(hydro_t* h, int64_t n, const float* positions, const float* orientations, int quat_xyzw,
                         const float* velocities, double dt, float* forces, float* torques, void* stream, const double* sea_time,
                         bool irr_entry = false)
{
    const float* orientations_wxyz = orientations;
    if (sea_time) { const int bad = check_sea_time(h, *sea_time); if (bad) return bad; }
    if (h && n > ((int64_t)1 << 26)) return fail(h, HYDRO_E_ARG, "array-of-structs entry handles at most 2^26 bodies per call");
    int rc = check_common(h, n);
    if (rc) return rc;
    if (!positions || !orientations_wxyz || !velocities || !forces || !torques) return fail(h, HYDRO_E_ARG, "null tensor pointer");
    if (!(dt > 0.0)) return fail(h, HYDRO_E_ARG, "dt must be > 0");
    if (!aligned_to(positions, 16) || !aligned_to(orientations_wxyz, 16) || !aligned_to(velocities, 16) ||
        !aligned_to(forces, 16) || !aligned_to(torques, 16))
        return fail(h, HYDRO_E_ARG, "array-of-structs tensors must be 16-byte aligned");
    if (n == 0) return HYDRO_OK;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    IrregularWater irr;                                                     // (the last refusal, before anything is written)
    if (irr_entry && (rc = irregular_water(h, n, irr))) return rc;
    if ((rc = prev_acquire(h, hydro_engine::kPrevTiled, n, s))) return rc;
    if (irr.table) launch_wrench_aos_irr(h, s, n, positions, orientations, quat_xyzw, velocities, dt, forces, torques, *sea_time, irr);
    else if (sea_time && h->sea_waves >= 0) launch_wrench_aos_sea(h, s, n, positions, orientations, quat_xyzw, velocities, dt, forces, torques, *sea_time);
    else dispatch_flags([&](auto HALF, auto NT, auto WARP) {
        hipLaunchKernelGGL((wrench_aos_direct_kernel<HALF, NT, WARP>), dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s,
                           positions, orientations, velocities, forces, torques, h->prev_tiled, h->params_tiled, quat_xyzw ? 1 : 0, (uint32_t)n,
                           h->semantics, h->rho, h->g, 1.0 / dt);
    }, h->half_coeffs, streaming(h, n), is_warp(h));
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}
}  // namespace

extern "C" {

int hydro_step_wrench_aos(hydro_t* h, int64_t n, const float* positions, const float* orientations, int quat_xyzw,
                          const float* velocities, double dt, float* forces, float* torques, void* stream)
{
    return step_wrench_aos_impl(h, n, positions, orientations, quat_xyzw, velocities, dt, forces, torques, stream, nullptr);
}

int hydro_step_wrench_aos_sea(hydro_t* h, int64_t n, const float* positions, const float* orientations, int quat_xyzw,
                              const float* velocities, double dt, float* forces, float* torques, double time, void* stream)
{
    return step_wrench_aos_impl(h, n, positions, orientations, quat_xyzw, velocities, dt, forces, torques, stream, &time);
}

int hydro_step_wrench_aos_irr(hydro_t* h, int64_t n, const float* positions, const float* orientations, int quat_xyzw,
                              const float* velocities, double dt, float* forces, float* torques, double time, void* stream)
{
    return step_wrench_aos_impl(h, n, positions, orientations, quat_xyzw, velocities, dt, forces, torques, stream, &time, true);
}

int hydro_step_components(hydro_t* h, int64_t n, const float* const state[HYDRO_STATE_FIELDS],
                          const float* const accel[HYDRO_PREV_FIELDS], float* const comps[HYDRO_COMP_FIELDS],
                          float* ratio, void* stream)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (!state || !accel || !comps) return fail(h, HYDRO_E_ARG, "null pointer table");
    if (n == 0) return HYDRO_OK;
    CompArgs a;
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) { if (!state[f]) return fail(h, HYDRO_E_ARG, "null state field"); a.st[f] = state[f]; }
    for (int f = 0; f < HYDRO_PREV_FIELDS; ++f) { if (!accel[f]) return fail(h, HYDRO_E_ARG, "null acceleration field"); a.acc[f] = accel[f]; }
    for (int f = 0; f < HYDRO_COMP_FIELDS; ++f) { if (!comps[f]) return fail(h, HYDRO_E_ARG, "null component field"); a.out[f] = comps[f]; }
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = ensure_soa_params(h))) return rc;
    fill_params(h, a);
    a.ratio = ratio; a.rho = h->rho; a.g = h->g; a.warp = h->semantics; a.n = n;
    const int grid = grid_for(n, kBlock);
    if (h->half_coeffs) hipLaunchKernelGGL(components_kernel<true>, dim3(grid), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(components_kernel<false>, dim3(grid), dim3(kBlock), 0, s, a);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

static int ke_launch(hydro_engine* h, KeArgs& a, int64_t n, int rotational, double* out_dev, void* stream)
{
    a.prm = h->params_tiled; a.prm_tile_floats = prm_tile_floats(h); a.mass_field = prm_mass_field(h);
    a.partials = h->ke_partials; a.partial_stride = h->ke_stride; a.out = out_dev; a.n = (uint32_t)n;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) return ke_of_nothing(h, out_dev, s);
    if (int rc = ke_prepare(h, s)) return rc;
    const dim3 grid(grid_for(n, kBlock)), blk(kBlock);
    if (rotational) hipLaunchKernelGGL(ke_kernel<true>, grid, blk, 0, s, a);
    else hipLaunchKernelGGL(ke_kernel<false>, grid, blk, 0, s, a);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int hydro_step_components_aos(hydro_t* h, int64_t n, const float* position, const float* orientation_xyzw,
                              const float* linear_vel, const float* angular_vel, const float* linear_accel,
                              const float* angular_accel, float* const out[8], float* ratio, void* stream)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (!position || !orientation_xyzw || !linear_vel || !angular_vel || !linear_accel || !angular_accel || !out)
        return fail(h, HYDRO_E_ARG, "null tensor pointer");
    if (n > ((int64_t)1 << 26)) return fail(h, HYDRO_E_ARG, "at most 2^26 bodies per call");
    if (n == 0) return HYDRO_OK;
    CompAosArgs a;
    a.pos = position; a.quat_xyzw = orientation_xyzw; a.lin_vel = linear_vel; a.ang_vel = angular_vel;
    a.lin_acc = linear_accel; a.ang_acc = angular_accel; a.prm = h->params_tiled;
    for (int k = 0; k < 8; ++k) { if (!out[k]) return fail(h, HYDRO_E_ARG, "null output tensor"); a.out[k] = out[k]; }
    a.ratio = ratio; a.rho = h->rho; a.g = h->g; a.warp = h->semantics; a.n = (uint32_t)n;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int grid = grid_for(n, kBlock);
    if (h->half_coeffs) hipLaunchKernelGGL(components_aos_kernel<true>, dim3(grid), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(components_aos_kernel<false>, dim3(grid), dim3(kBlock), 0, s, a);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

int hydro_kinetic_energy(hydro_t* h, int64_t n, const float* const state[HYDRO_STATE_FIELDS], int rotational,
                         double* out_dev, void* stream)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (!state || !out_dev) return fail(h, HYDRO_E_ARG, "null pointer");
    KeArgs a;
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) { if (!state[f]) return fail(h, HYDRO_E_ARG, "null state field"); a.st[f] = state[f]; }
    a.st_stride = 0; a.shift = 31; a.mask = 0xffffffffu;
    return ke_launch(h, a, n, rotational, out_dev, stream);
}

int hydro_kinetic_energy_tiled(hydro_t* h, int64_t n, const float* state, int64_t state_tile_stride, int rotational,
                               double* out_dev, void* stream)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (!out_dev) return fail(h, HYDRO_E_ARG, "null pointer");
    if ((rc = check_tiled(h, n, state, state_tile_stride, HYDRO_STATE_FIELDS, "null state"))) return rc;
    KeArgs a;
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) a.st[f] = state + f * HYDRO_TILE;
    a.st_stride = (uint32_t)state_tile_stride; a.shift = 6; a.mask = 63u;
    return ke_launch(h, a, n, rotational, out_dev, stream);
}

int hydro_integrate(hydro_t* h, int64_t n, const float* const state_in[HYDRO_STATE_FIELDS],
                    const float* const wrench[HYDRO_WRENCH_FIELDS], double dt,
                    float* const state_out[HYDRO_STATE_FIELDS], void* stream)
{
    int rc = check_common(h, n);
    if (rc) return rc;
    if (!state_in || !wrench || !state_out) return fail(h, HYDRO_E_ARG, "null pointer table");
    if (!(dt > 0.0)) return fail(h, HYDRO_E_ARG, "dt must be > 0");
    if (n == 0) return HYDRO_OK;
    IntArgs a;
    for (int f = 0; f < HYDRO_STATE_FIELDS; ++f) {
        if (!state_in[f] || !state_out[f]) return fail(h, HYDRO_E_ARG, "null state field");
        a.si[f] = state_in[f]; a.so[f] = state_out[f];
    }
    for (int f = 0; f < HYDRO_WRENCH_FIELDS; ++f) { if (!wrench[f]) return fail(h, HYDRO_E_ARG, "null wrench field"); a.w[f] = wrench[f]; }
    a.prm = h->params_tiled; a.prm_tile_floats = prm_tile_floats(h); a.mass_field = prm_mass_field(h);
    a.si_stride = a.w_stride = a.so_stride = 0; a.shift = 31; a.mask = 0xffffffffu;
    a.g = h->g; a.dt = (float)dt; a.n = (uint32_t)n;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(integrate_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, a);
    HYDRO_HIP(h, hipGetLastError(), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

// RCCL is bound lazily: a single-GPU user of libhydro.so needs no RCCL at all.  A communicator belongs to ONE copy of the
// library, so the ncclAllReduce to call is the one of the copy that made the caller's communicator:
//   1. the address the caller handed over (hydro_bind_rccl: `hydro_bind_rccl((void*)ncclAllReduce)` from C, the symbol of
//      the library object torch loaded from Python) - no guessing;
//   2. else HYDRO_RCCL_LIBRARY, if set: that library or nothing;
//   3. else the copy the process already has (dlsym over the global scope), else the system librccl.
// Only SUCCESS is latched: a first call before any RCCL is loaded fails with HYDRO_E_STATE and the next one looks again.
namespace {
typedef int (*nccl_all_reduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef const char* (*nccl_error_string_fn)(int);
std::mutex g_nccl_mutex;                              // (handles are independent across host threads)
nccl_all_reduce_fn g_nccl_all_reduce = nullptr;       // written once, under the mutex
nccl_error_string_fn g_nccl_error_string = nullptr;
const char* g_nccl_origin = "unbound";
constexpr int kNcclFloat64 = 8, kNcclSum = 0;        // rccl.h: ncclDataType_t / ncclRedOp_t (checked below when the header is there)

nccl_all_reduce_fn lookup_rccl(nccl_error_string_fn* err_fn, const char** origin)
{
    void* lib = nullptr;
    const char* named = getenv("HYDRO_RCCL_LIBRARY");
    void* sym = named ? nullptr : dlsym(RTLD_DEFAULT, "ncclAllReduce");
    *origin = "the copy already loaded in the process";
    if (!sym) {
        const char* candidates[] = {named, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* c : candidates) {
            if (!c) continue;
            if ((lib = dlopen(c, RTLD_NOW | RTLD_GLOBAL))) { *origin = (c == named) ? "HYDRO_RCCL_LIBRARY" : "librccl opened by libhydro"; break; }
            if (c == named) return nullptr;           // the one that was asked for, or nothing
        }
        if (!lib) return nullptr;
        sym = dlsym(lib, "ncclAllReduce");
    }
    *err_fn = reinterpret_cast<nccl_error_string_fn>(lib ? dlsym(lib, "ncclGetErrorString") : dlsym(RTLD_DEFAULT, "ncclGetErrorString"));
    return reinterpret_cast<nccl_all_reduce_fn>(sym);
}

nccl_all_reduce_fn bound_rccl(nccl_error_string_fn* error_string)
{
    std::lock_guard<std::mutex> lock(g_nccl_mutex);
    if (!g_nccl_all_reduce) {
        nccl_error_string_fn err_fn = nullptr;
        const char* origin = "unbound";
        if (nccl_all_reduce_fn fn = lookup_rccl(&err_fn, &origin)) { g_nccl_error_string = err_fn; g_nccl_origin = origin; g_nccl_all_reduce = fn; }
    }
    *error_string = g_nccl_error_string;
    return g_nccl_all_reduce;
}
}  // namespace

#if defined(__has_include)
#if __has_include(<rccl/rccl.h>)
}  // extern "C"
#include <rccl/rccl.h>
static_assert((int)ncclFloat64 == kNcclFloat64 && (int)ncclSum == kNcclSum, "rccl.h moved ncclFloat64 / ncclSum");
extern "C" {
#endif
#endif

int hydro_bind_rccl(void* nccl_all_reduce, void* nccl_get_error_string)
{
    std::lock_guard<std::mutex> lock(g_nccl_mutex);
    if (!nccl_all_reduce) {                            // forget: the next hydro_ke_allreduce looks the library up again
        g_nccl_all_reduce = nullptr; g_nccl_error_string = nullptr; g_nccl_origin = "unbound";
        return HYDRO_OK;
    }
    g_nccl_all_reduce = reinterpret_cast<nccl_all_reduce_fn>(nccl_all_reduce);
    g_nccl_error_string = reinterpret_cast<nccl_error_string_fn>(nccl_get_error_string);
    g_nccl_origin = "hydro_bind_rccl";
    return HYDRO_OK;
}

const char* hydro_rccl_origin(void)
{
    std::lock_guard<std::mutex> lock(g_nccl_mutex);
    return g_nccl_origin;
}

int hydro_ke_allreduce(hydro_t* h, void* nccl_comm, double* ke_dev, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    if (!nccl_comm || !ke_dev) return fail(h, HYDRO_E_ARG, "null communicator or buffer");
    nccl_error_string_fn error_string = nullptr;
    const nccl_all_reduce_fn all_reduce = bound_rccl(&error_string);
    if (!all_reduce) return fail(h, HYDRO_E_STATE, "RCCL is not available in this process (no ncclAllReduce loaded, librccl.so not found; hydro_bind_rccl hands one over, HYDRO_RCCL_LIBRARY names one)");
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    // in place, two doubles: [translational, rotational] (ncclAllReduce(count = 1..2, ncclDouble, ncclSum))
    const int rc = all_reduce(ke_dev, ke_dev, 2, kNcclFloat64, kNcclSum, nccl_comm, static_cast<hipStream_t>(stream));
    if (rc != 0) {
        snprintf(h->err, sizeof h->err, "ncclAllReduce: %s", error_string ? error_string(rc) : "failed");
        return HYDRO_E_LAUNCH;
    }
    return HYDRO_OK;
}

int hydro_ke_rearm(hydro_t* h, void* stream)
{
    if (!h) return HYDRO_E_ARG;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    HYDRO_HIP(h, hipMemsetAsync(ke_counters(h), 0, kKeCounterBytes, static_cast<hipStream_t>(stream)), HYDRO_E_LAUNCH);
    h->ke_suspect = false;
    return HYDRO_OK;
}

// HYDRO_ENABLE_TEST_HOOKS=1 in the environment WHEN THE LIBRARY IS LOADED (read once, by the static initialiser): the only
// way to make hydro_debug_ke_fault do anything.  A host that merely binds the library cannot corrupt a live engine with it.
static const bool g_test_hooks = [] { const char* v = getenv("HYDRO_ENABLE_TEST_HOOKS"); return v && v[0] == '1' && v[1] == 0; }();

int hydro_debug_ke_fault(hydro_t* h, int counter, uint32_t value, int as_failed_launch)
{
    if (!h) return HYDRO_E_ARG;
    if (!g_test_hooks) return fail(h, HYDRO_E_STATE, "hydro_debug_ke_fault is a test hook: refused unless HYDRO_ENABLE_TEST_HOOKS=1 was set when the library was loaded");
    if (counter < 0 || counter > (int)kKeClasses) return fail(h, HYDRO_E_ARG, "counter must be 0 (top) .. 64 (class 63)");
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    HYDRO_HIP(h, hipDeviceSynchronize(), HYDRO_E_LAUNCH);
    if (hipMemcpy(ke_counters(h) + 64 * counter, &value, sizeof value, hipMemcpyHostToDevice) != hipSuccess)
        return fail(h, HYDRO_E_LAUNCH, "hydro_debug_ke_fault: copy failed");
    if (as_failed_launch) h->ke_suspect = true;        // what fail() does when a HIP call of this handle reports an error
    return HYDRO_OK;
}

int hydro_set_semantics(hydro_t* h, int semantics)
{
    if (!h) return HYDRO_E_ARG;
    if (semantics != HYDRO_SEM_NUMBA && semantics != HYDRO_SEM_WARP)
        return fail(h, HYDRO_E_ARG, "semantics must be HYDRO_SEM_NUMBA (0) or HYDRO_SEM_WARP (1)");
    if (semantics == HYDRO_SEM_WARP) {
        // said once per process: what pins this mode is warp_hydrodynamics.py executed under a stand-in for the Warp runtime
        // (tests/test_warp_semantics.py), not NVIDIA's runtime, its fp32 rounding or its own quat_rotate (include/hydro.h)
        static std::once_flag told;               // (handles are independent across host threads)
        if (!getenv("HYDRO_QUIET"))
            std::call_once(told, [] {
                fprintf(stderr, "[libhydro] HYDRO_SEM_WARP: pinned on warp_hydrodynamics.py executed under an fp64 stand-in for the "
                                "Warp runtime (matrix quat_rotate), not on NVIDIA's runtime; HYDRO_SEM_NUMBA is the parity target\n");
            });
    }
    h->semantics = semantics;
    return HYDRO_OK;
}

int hydro_set_tuning(hydro_t* h, int bodies_per_lane, int block_threads, int non_temporal, int waves_per_simd)
{
    if (!h) return HYDRO_E_ARG;
    if (!(bodies_per_lane == 0 || bodies_per_lane == 1 || bodies_per_lane == 2))
        return fail(h, HYDRO_E_ARG, "bodies_per_lane must be 0, 1 or 2");
    if (!(block_threads == 0 || block_threads == 128 || block_threads == 256))
        return fail(h, HYDRO_E_ARG, "block_threads must be 0, 128 or 256");
    if (non_temporal < -1 || non_temporal > 1) return fail(h, HYDRO_E_ARG, "non_temporal must be -1, 0 or 1");
    if (waves_per_simd < -1 || waves_per_simd > 8) return fail(h, HYDRO_E_ARG, "waves_per_simd must be -1 .. 8");
    h->vec = bodies_per_lane;
    h->block = block_threads;
    h->nt = non_temporal;
    h->waves = waves_per_simd;
    return HYDRO_OK;
}

int hydro_sync(hydro_t* h)
{
    if (!h) return HYDRO_E_ARG;
    HYDRO_HIP(h, use_device(h->device), HYDRO_E_DEVICE);
    HYDRO_HIP(h, hipStreamSynchronize(h->stream), HYDRO_E_LAUNCH);
    return HYDRO_OK;
}

void* hydro_stream(hydro_t* h) { return h ? static_cast<void*>(h->stream) : nullptr; }

}  // extern "C"

namespace {
// (see their declarations: last in the file on purpose)
void launch_wrench_tiled_sea(hydro_engine* h, dim3 grid, dim3 blk, size_t lds, hipStream_t s, const float* state, const float* pv,
                             float* wrench, float* pv_out, uint32_t st_stride, uint32_t pv_stride, uint32_t out_stride, uint32_t pvo_stride,
                             int64_t n, double dt, bool own_prev, double time)
{
    dispatch_flags([&](auto HALF, auto WP, auto NT, auto WARP) {
        hipLaunchKernelGGL((wrench_tiled_sea_kernel<HALF, WP, NT, WARP>), grid, blk, lds, s,
                           state, pv, h->params_tiled, wrench, pv_out, st_stride, pv_stride, out_stride, pvo_stride,
                           (uint32_t)n, h->semantics, h->rho, h->g, 1.0 / dt,
                           (const void*)h->sea_table, (uint32_t)h->sea_waves, sea_step(time), time);
    }, h->half_coeffs, own_prev, streaming(h, n), is_warp(h));
}

void launch_wrench_aos_sea(hydro_engine* h, hipStream_t s, int64_t n, const float* positions, const float* orientations, int quat_xyzw,
                           const float* velocities, double dt, float* forces, float* torques, double time)
{
    dispatch_flags([&](auto HALF, auto NT, auto WARP) {
        hipLaunchKernelGGL((wrench_aos_sea_kernel<HALF, NT, WARP>), dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s,
                           positions, orientations, velocities, forces, torques, h->prev_tiled, h->params_tiled, quat_xyzw ? 1 : 0, (uint32_t)n,
                           h->semantics, h->rho, h->g, 1.0 / dt,
                           (const void*)h->sea_table, (uint32_t)h->sea_waves, sea_step(time), time);
    }, h->half_coeffs, streaming(h, n), is_warp(h));
}

void launch_wrench_tiled_irr(hydro_engine* h, dim3 grid, dim3 blk, size_t lds, hipStream_t s, const float* state, const float* pv,
                             float* wrench, float* pv_out, uint32_t st_stride, uint32_t pv_stride, uint32_t out_stride, uint32_t pvo_stride,
                             int64_t n, double dt, bool own_prev, double time, const IrregularWater& w)
{
    dispatch_flags([&](auto HALF, auto WP, auto NT, auto WARP, auto DEPTH) {
        const auto launch = [&](auto kernel, auto... depth) {
            hipLaunchKernelGGL(kernel, grid, blk, lds, s,
                               state, pv, h->params_tiled, wrench, pv_out, st_stride, pv_stride, out_stride, pvo_stride,
                               (uint32_t)n, h->semantics, h->rho, h->g, 1.0 / dt,
                               w.table, w.waves, sea_step(time), time, w.tiles_per_sea, depth...);
        };
        // (the kernels take HYDRO_FD_PARAMS with DEPTH only: <..., true, float> has the depth as its last argument, <..., false> none)
        if constexpr (DEPTH) launch(wrench_tiled_irr_kernel<HALF, WP, NT, WARP, true, float>, w.neg_depth);
        else launch(wrench_tiled_irr_kernel<HALF, WP, NT, WARP, false>);
    }, h->half_coeffs, own_prev, streaming(h, n), is_warp(h), w.depth);
}

void launch_wrench_aos_irr(hydro_engine* h, hipStream_t s, int64_t n, const float* positions, const float* orientations, int quat_xyzw,
                           const float* velocities, double dt, float* forces, float* torques, double time, const IrregularWater& w)
{
    dispatch_flags([&](auto HALF, auto NT, auto WARP, auto DEPTH) {
        const auto launch = [&](auto kernel, auto... depth) {
            hipLaunchKernelGGL(kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s,
                               positions, orientations, velocities, forces, torques, h->prev_tiled, h->params_tiled, quat_xyzw ? 1 : 0, (uint32_t)n,
                               h->semantics, h->rho, h->g, 1.0 / dt,
                               w.table, w.waves, sea_step(time), time, w.tiles_per_sea, depth...);
        };
        // (as above: <..., true, float> takes the depth, <..., false> does not)
        if constexpr (DEPTH) launch(wrench_aos_irr_kernel<HALF, NT, WARP, true, float>, w.neg_depth);
        else launch(wrench_aos_irr_kernel<HALF, NT, WARP, false>);
    }, h->half_coeffs, streaming(h, n), is_warp(h), w.depth);
}
}  // namespace
