// The register-resident factor + inverse (chol_res.hip) as pq_factor_batched routes to it.
#pragma once
#include "capi_util.h"

#define PQ_RES_NMAX 288          // largest n (18 block rows of 16)
#define PQ_RES_LDMAX 320         // largest pitch
#define PQ_RES_PROF_BLOCKS 1024  // PQ_PROFILE builds: workgroups whose phase clocks are kept

namespace pq {
// the plain matrix p_scale P + (p_diag + sigma) I (no general rows, no box: the group capacitance, the
// low-rank capacitances, the IPMs' normal matrices) up to the resident size; the kernel's tile load has
// form_elem's row loop and box term folded away, every other form keeps k_factor / k_factor_sk
inline bool factor_res_supports(const pq_problem* pb) {
  return pb->n > 0 && pb->n <= PQ_RES_NMAX && pb->ld <= PQ_RES_LDMAX && pb->mg == 0 && pb->lb == nullptr;
}
// k_factor_sk's contract with invert != 0, one 512-thread workgroup per problem (no allocation,
// no synchronisation: legal during stream capture)
void factor_res_launch(int grid, hipStream_t stream, const pq_problem* pb, const pq_state* st, const int32_t* idx,
                       int nidx, const pq_settings* s, int invert);
}  // namespace pq
