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

}  // namespace bsk
