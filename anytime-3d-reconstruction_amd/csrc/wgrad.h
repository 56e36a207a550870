// Weight gradients (internal): what wgrad.hip and wgrad_phase.hip share besides the plan.
#pragma once
#include "common.h"
#include "wgrad_plan.h"

// wgrad_phase.hip: the phase-form kernel of a stride-2 layer on plan `p` (WG_PHASE); leaves p.splits slabs [64 cin][cout] for the reduce.
void vv_wgrad_phase_launch(const void *src, const void *g, float *slabs, int batch, int side, int cin, int cout, const WgradPlan &p,
                           hipStream_t st);

// wgrad.hip: out[i] = alpha * (sum of the slabs in split order) (+ out[i] with `accumulate`), by the reduce kernel wgrad_reduce_sliced picks.
void vv_wgrad_reduce_launch(const float *slabs, float *out, long n, int splits, float alpha, int accumulate, hipStream_t st);
