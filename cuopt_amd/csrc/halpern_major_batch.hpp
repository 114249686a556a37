// The burst of device-decided major iterations for the K LPs of a Halpern small-LP batch (cuoptamd_batch_set_halpern_device_major,
// docs/design/04d_halpern_mode.md "Bursts of a K-workgroup batch"): what kernels_resident.hip (the batch object and the host side of a
// burst) and kernels_halpern_major.hip (the kernels and their launch sites) share.  A member's restart is finished by the batch
// restart's own body (halpern_restart_finish_workgroup, resident_halpern_bodies.hpp) on the batch restart's own record.
#pragma once
#include "halpern_major.hpp"
#include "resident_common.hpp"

// One record per member in the batch's pinned burst block, written once per burst.  Workgroups find their LP through a list (the loop: one list
// per resident tier) or through the (LP, block) table of the restart.
struct HalpernBurstMember {
  HalpernResidentArgs run;          // the loop's record; run.target_steps is the FIRST period's target (period j: + j * period)
  pdlpdev_halpern_major_state* st;  // this member's block on the device
  const double* sc;                 // the evaluation's nine raw sums: the member's pinned scalar block, slot 32
  pdlpdev_halpern_major_record* ring;  // 16 records in pinned host memory
  pdlpdev_halpern_major_params p;
  double r_prev;                    // the host's r_prev (k_halpern_major_arm_batch)
  RestartView R;                    // k_restart_batch's view: candidate = the current iterate, scaled distances
  HalpernRestartArgs fin;           // k_halpern_restart_finish_batch's record (no clear; fin.g blocks of R); the distances go to st and the ring
};

extern "C" {
// the launches of a batch burst, enqueued on s (count members in list; per tier: tier_list); j: the period's number in the burst
int halpern_batch_burst_arm(hipStream_t s, const HalpernBurstMember* mem, const int* list, int count);
int halpern_batch_burst_loop(hipStream_t s, int device, int tier, const HalpernBurstMember* mem, const int* tier_list, int count, int32_t add_target);
int halpern_batch_burst_eval(hipStream_t s, int device, size_t lds, const MajorSmallArgs* args, const HalpernBurstMember* mem, const int* list, int count,
                             int32_t add_target);
int halpern_batch_burst_decide(hipStream_t s, const HalpernBurstMember* mem, const int* list, int count, int32_t j, int32_t add_target);
int halpern_batch_burst_restart(hipStream_t s, const HalpernBurstMember* mem, const int2* blk, int blocks, const int* list, int count, int32_t j);
}
