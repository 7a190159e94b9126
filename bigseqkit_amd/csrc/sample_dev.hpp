// The random draw of `sample` and `shuffle` (PARITY.md SAMPLE / SHUF):
//     draw(seed, g) = splitmix64(splitmix64((uint64)(int64)seed) ^ g),   g = 0-based index of the record in the WHOLE input.
// The fate of a record depends on (seed, g) and on nothing else: not on how the input is cut into shards, streamed in
// pieces or spread over GPUs.  For a fixed seed it is a bijection of g (splitmix64 is one, and so is the xor): two records
// never share a draw.  tests/sample_ref.py restates it; tests/golden/sample_fixtures.json pins values of it.
#pragma once
#include <cstdint>

#include "hash_dev.hpp"

namespace bsk {

__host__ __device__ __forceinline__ uint64_t sample_key(int64_t seed) { return hashdev::splitmix64((uint64_t)seed); }
__host__ __device__ __forceinline__ uint64_t sample_draw(uint64_t key, uint64_t g) { return hashdev::splitmix64(key ^ g); }
// `sample`: kept iff the upper 53 bits of the draw lie under T = ceil(fraction * 2^53) (computed once on the host)
__host__ __device__ __forceinline__ bool sample_keeps(uint64_t key, uint64_t g, uint64_t T) { return (sample_draw(key, g) >> 11) < T; }
// ... which is a closed interval of the draw itself, the form the kernels take (a bucket of `shuffle` is one too; lo > hi: empty):
// [0, (T << 11) - 1], and for T = 2^53 the shift wraps to 0 and the upper end to ~0 -- every draw
struct DrawInterval { uint64_t lo, hi; };
constexpr __host__ __device__ DrawInterval sample_interval(uint64_t T) { return T == 0 ? DrawInterval{1, 0} : DrawInterval{0, (T << 11) - 1}; }
namespace sample_interval_check {
constexpr bool same(uint64_t T, uint64_t d) { return (sample_interval(T).lo <= d && d <= sample_interval(T).hi) == ((d >> 11) < T); }
// the draws 0, (T << 11) - 1, T << 11 and ~0, where T has them (T = 0: no draw under it; T = 2^53: none at or above it)
constexpr bool holds(uint64_t T) {
    return same(T, 0) && same(T, ~0ull) && (T == 0 || same(T, (T << 11) - 1)) && (T >= (1ull << 53) || same(T, T << 11));
}
static_assert(holds(0) && holds(1) && holds(1ull << 52) && holds((1ull << 53) - 1) && holds(1ull << 53), "sample_interval");
static_assert(sample_interval(0).lo > sample_interval(0).hi && sample_interval(1ull << 53).hi == ~0ull, "sample_interval: none / all");
}  // namespace sample_interval_check

}  // namespace bsk
