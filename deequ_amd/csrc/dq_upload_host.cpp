// dq_upload_host.cpp -- the host half of dq_upload_to (include/dqscan.h): a chunk's host columns laid out as the
// byte images of caller-owned column buffers.  Where dq_upload copies what the producer wrote, an owned buffer holds
// the canonical form a deequ_amd Table has: a NULL row's value is 0 (a NULL string is empty, bytes under it are
// dropped), bitmap bits past the last row are 0, a nullable column without a bitmap gets one of all ones, the padding
// behind every buffer's rows is 0.  Dictionary indices are widened and range-checked as dq_upload does it, and
// decimal128 values are checked against their precision.  No HIP: dq_upload_to (dq_ingest.cpp) adds the pinned slot
// and the DMA; tests/upload_to_check.cpp drives this file alone under host sanitizers.
#include "dq_upload_host.h"

extern "C" {

dq_status dq_upload_payload(const dq_host_column* cols, int32_t n_cols, int64_t* value_bytes) {
  return dq::up::payload(cols, n_cols, value_bytes);
}

dq_status dq_upload_stage(const dq_host_column* cols, int32_t n_cols, const dq_upload_dest* dests, void* staging,
                          int64_t staging_bytes, int32_t host_threads, int64_t* positions, int64_t* staged_bytes) {
  return dq::up::stage(cols, n_cols, dests, staging, staging_bytes, host_threads, positions, staged_bytes);
}

}  // extern "C"
