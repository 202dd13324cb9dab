// hydro_watch.h - host half of the trajectory recorder's watch tables (hydro_set_watch).  Plain C++, no HIP: the library
// includes it, and tests/test_recorder.py compiles it for the CPU and checks it against a brute-force construction.
//
// A watch list is `count` strictly ascending body indices.  The multi-step kernel owns one tile of 64 bodies per wavefront,
// so what a wave needs is per TILE: a 64-bit mask of its watched lanes and the log column of the first of them (the
// exclusive prefix sum of the masks' popcounts).  Body bodies[j] then records into column j:
//     column = first[body / 64] + popcount(mask[body / 64] & ((1 << body % 64) - 1))
#ifndef HYDRO_WATCH_H
#define HYDRO_WATCH_H

#include <stdint.h>

#ifndef HYDRO_WATCH_MAX
#define HYDRO_WATCH_MAX 65536   /* bodies in one watch list (include/hydro.h) */
#endif

namespace hydro {

// 0 if `bodies` is a valid watch list for an engine of `capacity` bodies, else which rule it breaks:
// 1 = count out of range, 2 = index out of [0, capacity), 3 = not strictly ascending (unsorted or duplicate).
inline int watch_check(int64_t count, const int64_t* bodies, int64_t capacity)
{
    if (count < 1 || count > HYDRO_WATCH_MAX) return 1;
    for (int64_t j = 0; j < count; ++j) {
        if (bodies[j] < 0 || bodies[j] >= capacity) return 2;
        if (j > 0 && bodies[j] <= bodies[j - 1]) return 3;
    }
    return 0;
}

// Fill mask[tiles] and first[tiles] for a list watch_check accepted (tiles >= bodies[count - 1] / 64 + 1).
inline void watch_tables(int64_t count, const int64_t* bodies, int64_t tiles, uint64_t* mask, uint32_t* first)
{
    for (int64_t t = 0; t < tiles; ++t) mask[t] = 0;
    for (int64_t j = 0; j < count; ++j) mask[bodies[j] >> 6] |= (uint64_t)1 << (bodies[j] & 63);
    uint32_t seen = 0;
    for (int64_t t = 0; t < tiles; ++t) {
        first[t] = seen;
        seen += (uint32_t)__builtin_popcountll(mask[t]);
    }
}

}  // namespace hydro
#endif  /* HYDRO_WATCH_H */
