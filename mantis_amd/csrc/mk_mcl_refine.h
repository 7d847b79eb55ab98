// Monte Carlo localization, the modes refined on the grid lines and the set
// recentred on them (mantis_mcl_refine_modes, include/mantis.h): the plan of a
// call -- which modes are applied and the rigid correction of each -- and the
// move of one particle, shared by the device (k_mcl_recentre,
// mcl_refine_impl.hip) and the host build of the CPU tests (hostcheck.cpp
// hc_mcl_refine_plan / hc_mcl_recentre). The key rule is mk_mcl_modes.h's, the
// refinement's are mk_refine.h's, unchanged.
//
// Mode k with estimate T_mode,k was refined to T_ref,k. Its correction is the
// world-frame rigid motion X_k = T_ref,k T_mode,k^-1, so X_k T_mode,k = T_ref,k
// up to rounding. A mode is applied only when the refinement held (refined = 1)
// and the refined pose still has the mode's key against the anchor: a pose that
// left its cell is another mode's business. Particle j of the current set moves
// by X_k iff its key is an applied mode's bin; every other particle keeps its
// bits. xf_mul is the plain product (no re-orthonormalisation) and both builds
// keep -ffp-contract=off: host and device give the same bits.
#pragma once
#include "mk_mcl_modes.h"

namespace mk {
namespace mcl {

// What k_mcl_recentre gets as kernel arguments: the anchor, the grid spacing,
// per mode the bin (-1: not applied, matches no key) and the correction.
struct Recentre {
  Xf A;
  double g;
  int32_t n_modes, pad;
  int32_t bin[kMaxModes];
  Xf X[kMaxModes];
};

MK_HD Xf xf_identity() {
  Xf o;
  for (int e = 0; e < 9; e++) o.R[e] = (e % 4 == 0) ? 1.0 : 0.0;
  o.t[0] = o.t[1] = o.t[2] = 0.0;
  return o;
}

// The plan over the modes record O (anchor and keys as mantis_mcl_modes left
// them), T_ref / refined: the refinement's pose (16 doubles, row-major) and
// flag per mode. key_kept / applied: kMaxModes entries, zero past n_modes.
MK_HD void refine_plan(const Modes& O, double g, const double* T_ref, const int32_t* refined, int32_t apply,
                       int32_t* key_kept, int32_t* applied, Recentre* P) {
  P->A = track::xf_from_mat4(O.anchor_T_w_b);
  P->g = g;
  P->n_modes = O.n_modes < kMaxModes ? O.n_modes : kMaxModes;
  P->pad = 0;
  for (int k = 0; k < kMaxModes; k++) {
    key_kept[k] = applied[k] = 0;
    P->bin[k] = -1;
    P->X[k] = xf_identity();
    if (k >= P->n_modes) continue;
    const Mode& M = O.mode[k];
    const Xf Tr = track::xf_from_mat4(T_ref + 16 * k);
    int32_t ix, iy, q;
    const int32_t bin = cell_bin(M.ix, M.iy, M.yaw_quadrant);
    key_kept[k] = (refined[k] != 0 && cell_key(Tr, P->A, g, &ix, &iy, &q) == bin) ? 1 : 0;
    applied[k] = (apply != 0 && key_kept[k]) ? 1 : 0;
    P->X[k] = xf_mul(Tr, xf_inverse(track::xf_from_mat4(M.T_w_b)));
    if (applied[k]) P->bin[k] = bin;
  }
}

// Particle T of the current set under the plan: moved by the correction of the
// applied mode whose bin is T's key (returns that mode), or untouched (-1). The
// modes' bins are distinct, so at most one matches. The loop runs over the
// plan's entries by a uniform index: on the device they stay scalar operands.
MK_HD int32_t recentre_pose(const Recentre& P, Xf& T) {
  int32_t ix, iy, q;
  const int32_t b = cell_key(T, P.A, P.g, &ix, &iy, &q);  // >= 0
  const Xf T0 = T;
  int32_t hit = -1;
  for (int k = 0; k < kMaxModes; k++)
    if (k < P.n_modes && P.bin[k] == b) {
      T = xf_mul(P.X[k], T0);
      hit = k;
    }
  return hit;
}

}  // namespace mcl
}  // namespace mk
