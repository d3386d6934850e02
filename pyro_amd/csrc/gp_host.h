// gp_host.h -- what the launchers and entry points of the Gaussian-process kernels share on the host: the launch with
// dynamic LDS, the two-sided backward driver of the tiled kernels, and the argument checks that the pa_gp_*_bwd entry
// points have in common.  Every message carries the entry point's own name (``who``).
#pragma once
#include "common.h"
#include "gp_kernel_plan.h"

namespace pa {

// launch ``kernel`` on ``grid`` workgroups of ``threads`` with ``lds`` bytes of dynamic LDS (over 48 KiB the kernel's
// limit is raised first), then check_launch under ``name``
template <typename... P, typename... A>
static int gp_launch(const char* name, void (*kernel)(P...), int64_t grid, int threads, size_t lds, hipStream_t st,
                     const A&... args) {
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds, st, args...);
  return check_launch(name);
}

// One call of a tiled backward (GpkCallPlan): x's launch, then, for a z of its own that wants a gradient, z's with the
// roles exchanged (G read through transposed strides).  With z = x (null) x's launch gives x both roles (sym).  The
// reduced gradients come from the first launch that runs.
//   side(plan, rows' points, walked points, g_sr, g_sc, sym, scalars, workspace, g_rows) -> PA_OK or an error
template <typename T, typename SIDE>
static int gp_bwd_two_sided(const GpkCallPlan& cp, const void* x, const void* z, int64_t M, void* gx, void* gz,
                            bool any_scalar, void* workspace, const SIDE& side) {
  double* ws = (double*)workspace;
  if (cp.run_x) {
    int rc = side(cp.x, (const T*)x, (const T*)(z ? z : x), M, (int64_t)1, z == nullptr, any_scalar, ws, (T*)gx);
    if (rc != PA_OK) return rc;
  }
  if (cp.run_z)
    return side(cp.z, (const T*)z, (const T*)x, (int64_t)1, M, false, any_scalar && !cp.run_x, ws + cp.z_offset_doubles,
                (T*)gz);
  return PA_OK;
}

// The checks that pa_gp_kernel_bwd, pa_gp_periodic_bwd, pa_gp_dot_bwd and pa_gp_compose_bwd share, after the kernel's
// own: ``wanted`` says whether any gradient was asked for.  PA_OK with *launch = false: nothing to do.
static int gp_bwd_preamble(const char* who, const void* z, const void* gz, int forced_splits, bool wanted, int64_t N,
                           int64_t M, const void* G, bool* launch) {
  *launch = false;
  PA_REQUIRE(gz == nullptr || z != nullptr, "%s: gz without a z (with z = x, gx takes both roles)", who);
  PA_REQUIRE(forced_splits >= 0, "%s: forced_splits=%d", who, forced_splits);
  if (!wanted) return PA_OK;
  PA_REQUIRE(N > 0 && M > 0, "%s: an empty matrix has zero gradients; the caller fills them", who);
  PA_REQUIRE(G != nullptr, "%s: null G", who);
  *launch = true;
  return PA_OK;
}

// the records of EVERY launch of the call fit the workspace that was handed in (not merely one sized by the caller's flags)
static int gp_workspace_check(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
  PA_REQUIRE(workspace != nullptr && need <= workspace_bytes && (uintptr_t)workspace % 8 == 0,
             "%s: workspace of %zu bytes, the plan needs %zu (8-byte aligned)", who, workspace_bytes, need);
  return PA_OK;
}

}  // namespace pa
