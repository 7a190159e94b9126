// `faidx -d`: the fetch kernel over the tiles of a prepared batch (fai_fetch_dev.hpp, fai_fetch.hpp); DESIGN.md f21
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "fai_fetch_dev.hpp"

namespace bsk {

// buf: the batch's spans (fai::layout), padded; *status is fai::FETCH_NO_FAULT before the launch and the lowest violation of
// check 1 after it.  Every tile writes its own bytes of out[0, out_bytes) and nothing else.
hipError_t launch_faidx_fetch(const uint8_t* buf, const fai::FetchHit* hits, const fai::FetchTile* tiles, uint32_t ntiles,
                              uint32_t line_width, const uint8_t* comp, const uint8_t* headers, uint8_t* out, uint64_t* status,
                              int num_cus, hipStream_t st);

}  // namespace bsk
