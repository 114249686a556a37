// The three restart tests of the reflected-Halpern mode, once for the host (halpern_major_head, pdlp_solver.cpp) and for the device
// (halpern_major_decide, halpern_major.hpp).  No HIP in here: the host driver is compiled by the plain C++ compiler.
#pragma once
#ifdef __HIPCC__
#define HALPERN_HOST_DEVICE __host__ __device__
#else
#define HALPERN_HOST_DEVICE
#endif
// r_first, r_prev: r of the first step since the last restart and at the previous check since then (< 0: none); k: steps since then
HALPERN_HOST_DEVICE inline bool halpern_restart_due(double r, double r_first, double r_prev, int k, int total_iterations, double sufficient,
                                                    double necessary, double artificial)
{
  if (r <= sufficient * r_first) return true;
  else if (r <= necessary * r_first && r_prev >= 0.0 && r > r_prev) return true;
  else if ((double)k >= artificial * (double)total_iterations) return true;
  return false;
}
#undef HALPERN_HOST_DEVICE
