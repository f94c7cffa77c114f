// pp3_model.hip -- the env library's host model builder: pp3_model_t + pp3_env_config_t -> the
// DevModel record the kernels read (pp3_device.h), its per-lane phase records and pair tables.
// float64 host arithmetic only: no kernel, no HIP runtime call (pp3_create uploads the result).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "pp3_device.h"
#include "pp3_env_host.h"

using namespace pp3;
using namespace pp3::model_limits;  // HMAX, NROBOT_GEOM

static void clamp_solimp(const double in[5], float out[5]) {
  double dmin = in[0], dmax = in[1], width = in[2], mid = in[3], power = in[4];
  dmin = dmin < 0.0001 ? 0.0001 : dmin > 0.9999 ? 0.9999 : dmin;
  dmax = dmax < 0.0001 ? 0.0001 : dmax > 0.9999 ? 0.9999 : dmax;
  width = width < 1e-15 ? 1e-15 : width;
  mid = mid < 0.0001 ? 0.0001 : mid > 0.9999 ? 0.9999 : mid;
  power = power < 1 ? 1 : power;
  out[0] = (float)dmin; out[1] = (float)dmax; out[2] = (float)width; out[3] = (float)mid; out[4] = (float)power;
}
static void kb_of(const double solref[2], const double solimp[5], double h, float* k, float* b) {
  float si[5];
  clamp_solimp(solimp, si);
  double dmax = si[1];
  if (solref[0] > 0) {
    double tc = solref[0] < 2 * h ? 2 * h : solref[0], dr = solref[1];
    *k = (float)(1.0 / (dmax * dmax * tc * tc * dr * dr));
    *b = (float)(2.0 / (dmax * tc));
  } else {
    *k = (float)(-solref[0] / (dmax * dmax));
    *b = (float)(-solref[1] / dmax);
  }
}
static double imp_host(const float si[5], double pos, double margin) {
  double x = fabs((pos - margin) / si[2]);
  if (x >= 1) return si[1];
  if (x <= 0) return si[0];
  double y;
  if (si[4] == 1) y = x;
  else if (x <= si[3]) y = pow(x, si[4]) / pow(si[3], si[4] - 1);
  else y = 1 - pow(1 - x, si[4]) / pow(1 - si[3], si[4] - 1);
  return si[0] + y * (si[1] - si[0]);
}

void quat2mat_d(const double q[4], double R[9]) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

// the per-lane phase records (pp3_device.h LaneRec) from the already filled model fields
static void set_i(float& f, int32_t v) { memcpy(&f, &v, 4); }
template <int N>
static void put_rec(LaneTab<N>& t, int l, const LaneRec<N>& r) {
  for (int k = 0; k < N; k++)
    for (int c = 0; c < 4; c++) t.g[k][l][c] = r.f[4 * k + c];
}
static void fill_lane_records(DevModel* d) {
  for (int l = 0; l < 32; l++) {
    LaneRec<(LL_WORDS + 3) / 4> rl = {};
    float* f = rl.f;
    if (l < 2 * (NJ - 1)) {
      const int j = 1 + l / 2, hi = l & 1;
      set_i(f[LL_LIM_ON], d->jnt_limited[j] ? 1 : 0);
      f[LL_RANGE] = d->jnt_range[j][hi];
      f[LL_MARGIN] = d->lim_margin[j];
      f[LL_INVW] = d->lim_invw[j];
      f[LL_B] = d->lim_b[j];
      f[LL_K] = d->lim_k[j];
      for (int k = 0; k < 5; k++) f[LL_SOLIMP + k] = d->lim_solimp[j][k];
    }
    if (l < NFR) {
      f[LL_FR_R] = d->fr_R[6 + l];
      f[LL_FR_B] = d->fr_b[6 + l];
    }
    if (l < NU) {
      set_i(f[LL_ACT_DOF], d->act_dof[l]);
      set_i(f[LL_ACT_QADR], d->act_qadr[l]);
      set_i(f[LL_ACT_FLAGS], (d->act_ctrllimited[l] ? ACTF_CTRLLIMITED : 0) | (d->act_forcelimited[l] ? ACTF_FORCELIMITED : 0) |
                                 (d->act_biastype[l] == PP3_BIAS_AFFINE ? ACTF_AFFINE : 0));
      f[LL_CRANGE] = d->act_crange[l][0];
      f[LL_CRANGE + 1] = d->act_crange[l][1];
      f[LL_GEAR] = d->act_gear[l];
      f[LL_GAIN] = d->act_gain[l];
      for (int k = 0; k < 3; k++) f[LL_BIAS + k] = d->act_bias[l][k];
      f[LL_FRANGE] = d->act_frange[l][0];
      f[LL_FRANGE + 1] = d->act_frange[l][1];
    }
    LaneRec<(LC_WORDS + 3) / 4> rc = {};
    float* c = rc.f;
    if (l >= 1 && l < NB)
      for (int k = 0; k < 4; k++) c[LC_IQUAT + k] = d->body_iquat[l][k];
    if (l < d->nrobot_geom) {
      const int g = d->robot_geom[l];
      set_i(c[LC_PT_BODY], d->cg_body[g]);
      for (int k = 0; k < 3; k++) c[LC_PT_POS + k] = d->cg_pos[g][k];
    } else if (l >= 16 && l < 20) {
      const int si = d->feet_site[l - 16];
      set_i(c[LC_PT_BODY], d->site_body[si]);
      for (int k = 0; k < 3; k++) c[LC_PT_POS + k] = d->site_pos[si][k];
    }
    LaneRec<(LM_WORDS + 3) / 4> rm = {};
    float* mr = rm.f;
    for (int t = 0; t < 4; t++) {
      const int p = l + 32 * t;
      if (p < d->nmpair) {
        const int i = d->mp_i[p], j = d->mp_j[p];
        set_i(mr[LM_IJ + t], i | (j << 8));
        mr[LM_ARM + t] = i == j ? d->dof_armature[i] : 0.0f;
      } else {
        set_i(mr[LM_IJ + t], -1);
      }
    }
    if (l < NV) mr[LM_DAMP] = d->dof_damping[l];
    if (l < NFR) mr[LM_FLOSS] = d->fr_floss[6 + l];
    LaneRec<(LE_WORDS + 3) / 4> re = {};
    float* e = re.f;
    if (l < NU) {
      e[LE_POSE] = d->default_pose[l];
      e[LE_JLO] = d->jlo[l];
      e[LE_JHI] = d->jhi[l];
      if (l % 3 == 1) e[LE_ABD] = d->des_abd[l / 3];
    }
    if (l < 4) set_i(e[LE_LEG], d->lower_leg_body[l]);
    if (l >= 16 && l < 16 + NU) e[LE_POSE16] = d->default_pose[l - 16];
    put_rec(d->lane_lim, l, rl);
    put_rec(d->lane_com, l, rc);
    put_rec(d->lane_m, l, rm);
    put_rec(d->lane_env, l, re);
    LaneRec<(LS_WORDS + 3) / 4> rs = {};
    float* sr = rs.f;
    if (l < d->nsensor) {
      const int sid = d->sensor_objid[l], b = d->site_body[sid];
      set_i(sr[LS_TYPE], d->sensor_type[l]);
      set_i(sr[LS_ADR], d->sensor_adr[l]);
      sr[LS_CUT] = d->sensor_cutoff[l];
      set_i(sr[LS_BODY], b);
      for (int k = 0; k < 3; k++) sr[LS_SPOS + k] = d->site_pos[sid][k];
      for (int k = 0; k < 4; k++) sr[LS_SQUAT + k] = d->site_quat[sid][k];
      int chain[NB], n = 0;  // (depth checked at create)
      for (int bb = b; bb > 0 && n < LS_MAXCH; bb = d->body_parent[bb]) chain[n++] = bb;
      set_i(sr[LS_NCH], n);
      for (int c = 0; c < n; c++) {  // root first
        const int bb = chain[n - 1 - c];
        set_i(sr[LS_CH + 4 * c], bb);
        set_i(sr[LS_CH + 4 * c + 1], d->body_dofadr[bb]);
        set_i(sr[LS_CH + 4 * c + 2], d->body_dofnum[bb]);
        set_i(sr[LS_CH + 4 * c + 3], d->body_parent[bb]);
      }
    }
    put_rec(d->lane_sens, l, rs);
  }
  for (int p = 0; p < d->npair; p++) {
    d->pair_gid[p][0] = (float)d->cg_id[d->pair_g1[p]];
    d->pair_gid[p][1] = (float)d->cg_id[d->pair_g2[p]];
  }
  for (int p = 0; p < d->npair; p++) {
    const int ga = d->cg_id[d->pair_g1[p]], gb = d->cg_id[d->pair_g2[p]];
    int kn = 0, bo = 0;
    for (int i = 0; i < d->n_knee_geoms; i++) kn += (ga == d->knee_geoms[i] || gb == d->knee_geoms[i]) ? 1 : 0;
    for (int i = 0; i < d->n_torso_geoms; i++) bo += (ga == d->torso_geoms[i] || gb == d->torso_geoms[i]) ? 1 : 0;
    d->pair_con[p].knee = (float)kn;
    d->pair_con[p].body = (float)bo;
  }
}

int build_devmodel(const pp3_model_t* mm, const pp3_env_config_t* c, DevModel* d) {
  memset(d, 0, sizeof(*d));
  // topology checks (fixed-structure kernel)
  if (mm->jnt_type[0] != PP3_JNT_FREE || mm->body_parentid[1] != 0) return set_err(PP3_ERR_MODEL, "base must be a free body");
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) {
      int b = 2 + 3 * l + k, j = 1 + 3 * l + k;
      if (mm->body_parentid[b] != (k == 0 ? 1 : b - 1) || mm->body_jntadr[b] != j || mm->jnt_type[j] != PP3_JNT_HINGE ||
          mm->jnt_dofadr[j] != 6 + 3 * l + k || mm->jnt_qposadr[j] != 7 + 3 * l + k)
        return set_err(PP3_ERR_MODEL, "legs must be 4 serial chains of 3 hinge bodies");
    }
  if (mm->cone != PP3_CONE_PYRAMIDAL) return set_err(PP3_ERR_MODEL, "only pyramidal cones");
  for (int j = 1; j < NJ; j++)
    if (mm->jnt_pos[j][0] != 0 || mm->jnt_pos[j][1] != 0 || mm->jnt_pos[j][2] != 0)
      return set_err(PP3_ERR_MODEL, "hinge anchors must coincide with body origins (jnt_pos = 0)");
  if (mm->eulerdamp) {
    for (int i = 0; i < NV; i++)
      if (mm->dof_damping[i] > 0) return set_err(PP3_ERR_MODEL, "eulerdamp with joint damping is not supported (xml:58 disables it)");
  }
  if (c->obs_history < 1 || c->obs_history > HMAX) return set_err(PP3_ERR_ARG, "observation_history must be in [1, 16]");
  if (c->latency_len < 1 || c->latency_len > PP3_MAX_LAG || c->imu_latency_len < 1 || c->imu_latency_len > PP3_MAX_LAG)
    return set_err(PP3_ERR_ARG, "latency distributions must have 1..8 entries");
  if (c->n_frames < 1) return set_err(PP3_ERR_ARG, "n_frames < 1");
  const double h = mm->timestep;
  d->h = (float)h;
  for (int k = 0; k < 3; k++) d->gravity[k] = (float)mm->gravity[k];
  d->impratio = (float)mm->impratio;
  d->gtol_scale = (float)(mm->tolerance * mm->ls_tolerance * mm->meaninertia * NV);
  d->ls_iterations = mm->ls_iterations;
  d->iterations = mm->iterations;
  for (int b = 0; b < NB; b++) {
    for (int k = 0; k < 3; k++) {
      d->body_pos[b][k] = (float)mm->body_pos[b][k];
      d->body_ipos[b][k] = (float)mm->body_ipos[b][k];
      d->body_inertia[b][k] = (float)mm->body_inertia[b][k];
    }
    for (int k = 0; k < 4; k++) {
      d->body_quat[b][k] = (float)mm->body_quat[b][k];
      d->body_iquat[b][k] = (float)mm->body_iquat[b][k];
    }
    d->body_mass[b] = (float)mm->body_mass[b];
    uint32_t mask = 0;
    for (int bb = b; bb > 0; bb = mm->body_parentid[bb])
      for (int i = 0; i < mm->body_dofnum[bb]; i++) mask |= 1u << (mm->body_dofadr[bb] + i);
    d->body_dofmask[b] = mask;
  }
  for (int i = 0; i < NV; i++) d->dof_body[i] = mm->dof_bodyid[i];
  for (int j = 0; j < NJ; j++) {
    for (int k = 0; k < 3; k++) {
      d->jnt_pos[j][k] = (float)mm->jnt_pos[j][k];
      d->jnt_axis[j][k] = (float)mm->jnt_axis[j][k];
    }
    d->jnt_range[j][0] = (float)mm->jnt_range[j][0];
    d->jnt_range[j][1] = (float)mm->jnt_range[j][1];
    d->jnt_limited[j] = mm->jnt_limited[j];
    kb_of(mm->jnt_solref[j], mm->jnt_solimp[j], h, &d->lim_k[j], &d->lim_b[j]);
    clamp_solimp(mm->jnt_solimp[j], d->lim_solimp[j]);
    d->lim_margin[j] = (float)mm->jnt_margin[j];
    d->lim_invw[j] = (float)mm->dof_invweight0[mm->jnt_dofadr[j]];
    // both sides of one hinge can only be violated together when the range is narrower than
    // twice the margin; excluding that bounds the limit rows at one per hinge (NLMAX)
    if (j > 0 && mm->jnt_limited[j] && !(mm->jnt_range[j][1] - mm->jnt_range[j][0] > 2.0 * mm->jnt_margin[j]))
      return set_err(PP3_ERR_MODEL, "joint " + std::to_string(j) +
                                        ": range narrower than twice the margin (both limit sides could be active)");
  }
  for (int i = 0; i < NQ; i++) { d->qpos0[i] = (float)mm->qpos0[i]; d->key_qpos[i] = (float)mm->key_qpos[i]; }
  for (int i = 0; i < NV; i++) {
    d->dof_armature[i] = (float)mm->dof_armature[i];
    d->dof_damping[i] = (float)mm->dof_damping[i];
    d->fr_floss[i] = (float)mm->dof_frictionloss[i];
    float si[5], k, b;
    clamp_solimp(mm->dof_solimp[i], si);
    kb_of(mm->dof_solref[i], mm->dof_solimp[i], h, &k, &b);
    double imp = imp_host(si, 0.0, 0.0);
    double R = (1 - imp) / imp * mm->dof_invweight0[i];
    d->fr_R[i] = (float)(R < 1e-15 ? 1e-15 : R);
    d->fr_b[i] = b;
    if (i >= 6 && mm->dof_frictionloss[i] <= 0) return set_err(PP3_ERR_MODEL, "every hinge needs frictionloss > 0 (xml:55)");
    if (i < 6 && mm->dof_frictionloss[i] > 0) return set_err(PP3_ERR_MODEL, "free-joint frictionloss unsupported");
  }
  // M sparsity pairs
  int np = 0;
  for (int i = 0; i < NV; i++)
    for (int j = i; j >= 0; j = mm->dof_parentid[j]) {
      if (np >= NMPAIR_MAX) return set_err(PP3_ERR_MODEL, "M too dense");
      d->mp_i[np] = (uint8_t)i;
      d->mp_j[np] = (uint8_t)j;
      np++;
    }
  d->nmpair = np;
  if (np != NMPAIR) return set_err(PP3_ERR_MODEL, "mass-matrix sparsity differs from the 13-body quadruped tree");
  // collision geoms
  d->ncgeom = mm->ncgeom;
  int nslot = 0;
  int box_slot[PP3_MAX_CGEOM];
  d->nbox = 0;
  d->terrain = 0;
  for (int g = 0; g < mm->ncgeom; g++) {
    box_slot[g] = (mm->cgeom_bodyid[g] == 0 && mm->cgeom_type[g] == PP3_GEOM_BOX) ? d->nbox++ : -1;
    d->cg_type[g] = mm->cgeom_type[g];
    d->cg_body[g] = mm->cgeom_bodyid[g];
    d->cg_id[g] = mm->cgeom_id[g];
    for (int k = 0; k < 3; k++) d->cg_size[g][k] = (float)mm->cgeom_size[g][k];
    if (mm->cgeom_bodyid[g] == 0) {
      d->cg_slot[g] = -1;
      double R[9];
      quat2mat_d(mm->cgeom_quat[g], R);
      for (int k = 0; k < 9; k++) d->cg_wmat[g][k] = (float)R[k];
      for (int k = 0; k < 3; k++) d->cg_pos[g][k] = (float)mm->cgeom_pos[g][k];
    } else {
      if (mm->cgeom_type[g] != PP3_GEOM_SPHERE) return set_err(PP3_ERR_MODEL, "moving collision geoms must be spheres");
      if (nslot >= NROBOT_GEOM) return set_err(PP3_ERR_MODEL, "too many robot collision geoms (max 8)");
      d->cg_slot[g] = nslot;
      d->robot_geom[nslot++] = g;
      for (int k = 0; k < 3; k++) d->cg_pos[g][k] = (float)mm->cgeom_pos[g][k];
    }
  }
  d->nrobot_geom = nslot;
  d->npair = mm->npair;
  for (int p = 0; p < mm->npair; p++) {
    int g1 = mm->pair_g1[p], g2 = mm->pair_g2[p];
    d->pair_g1[p] = g1;
    d->pair_g2[p] = g2;
    // mj_contactParam
    double solref[2], solimp[5], mu;
    int p1 = mm->cgeom_priority[g1], p2 = mm->cgeom_priority[g2];
    if (p1 != p2) {
      int g = p1 > p2 ? g1 : g2;
      mu = mm->cgeom_friction[g][0];
      for (int k = 0; k < 2; k++) solref[k] = mm->cgeom_solref[g][k];
      for (int k = 0; k < 5; k++) solimp[k] = mm->cgeom_solimp[g][k];
    } else {
      double s1 = mm->cgeom_solmix[g1], s2 = mm->cgeom_solmix[g2], mix;
      if (s1 >= 1e-15 && s2 >= 1e-15) mix = s1 / (s1 + s2);
      else if (s1 < 1e-15 && s2 < 1e-15) mix = 0.5;
      else if (s1 < 1e-15) mix = 0;
      else mix = 1;
      if (mm->cgeom_solref[g1][0] > 0 && mm->cgeom_solref[g2][0] > 0)
        for (int k = 0; k < 2; k++) solref[k] = mix * mm->cgeom_solref[g1][k] + (1 - mix) * mm->cgeom_solref[g2][k];
      else
        for (int k = 0; k < 2; k++) solref[k] = fmin(mm->cgeom_solref[g1][k], mm->cgeom_solref[g2][k]);
      for (int k = 0; k < 5; k++) solimp[k] = mix * mm->cgeom_solimp[g1][k] + (1 - mix) * mm->cgeom_solimp[g2][k];
      mu = fmax(mm->cgeom_friction[g1][0], mm->cgeom_friction[g2][0]);
    }
    d->pair_mu[p] = (float)mu;
    kb_of(solref, solimp, h, &d->pair_k[p], &d->pair_b[p]);
    clamp_solimp(solimp, d->pair_solimp[p]);
    d->pair_margin[p] = (float)(fmax(mm->cgeom_margin[g1], mm->cgeom_margin[g2]) - fmax(mm->cgeom_gap[g1], mm->cgeom_gap[g2]));
    d->pair_tran[p] = (float)(mm->body_invweight0[mm->cgeom_bodyid[g1]][0] + mm->body_invweight0[mm->cgeom_bodyid[g2]][0]);
    {  // column support of this pair's contact Jacobian (bodies 2..13 = legs of 3 links, 1 = base)
      auto cls = [](int b) { return b == 0 ? -1 : (b == 1 ? 4 : (b - 2) / 3); };
      const int c1 = cls(mm->cgeom_bodyid[g1]), c2 = cls(mm->cgeom_bodyid[g2]);
      int sup;
      if (c1 < 0) sup = c2;
      else if (c2 < 0) sup = c1;
      else if (c1 == c2) sup = c1;
      else if (c1 == 4) sup = c2;
      else if (c2 == 4) sup = c1;
      else sup = 5 | 8 | ((c1 < c2 ? c1 : c2) << 4) | ((c1 < c2 ? c2 : c1) << 6);  // leg-leg: the pair
      d->pair_sup[p] = sup < 0 ? 5 : sup;  // (5 without bit 3: legs unknown -> dense LDL^T)
    }
    d->pair_dm[p][0] = d->body_dofmask[mm->cgeom_bodyid[g1]];
    d->pair_dm[p][1] = d->body_dofmask[mm->cgeom_bodyid[g2]];
    {  // flattened narrow-phase record
      PairRec r;
      memset(&r, 0, sizeof(r));
      const int t1 = mm->cgeom_type[g1], t2 = mm->cgeom_type[g2];
      r.kind = (t1 == PP3_GEOM_PLANE && t2 == PP3_GEOM_SPHERE) ? PK_PLANE_SPHERE
               : (t1 == PP3_GEOM_SPHERE && t2 == PP3_GEOM_SPHERE) ? PK_SPHERE_SPHERE
               : (t1 == PP3_GEOM_SPHERE && t2 == PP3_GEOM_BOX) ? PK_SPHERE_BOX : -1;
      r.s1 = d->cg_slot[g1];
      r.s2 = r.kind == PK_SPHERE_BOX ? -1 - box_slot[g2] : d->cg_slot[g2];
      r.r1 = d->cg_size[g1][0];
      r.r2 = d->cg_size[g2][0];
      r.margin = d->pair_margin[p];
      for (int k = 0; k < 3; k++) { r.p1[k] = d->cg_pos[g1][k]; r.p2[k] = d->cg_pos[g2][k]; }
      const int gf = r.kind == PK_SPHERE_BOX ? g2 : g1;  // plane frame / box frame
      for (int k = 0; k < 9; k++) r.R[k] = d->cg_wmat[gf][k];
      if (r.kind == PK_SPHERE_BOX)
        for (int k = 0; k < 3; k++) r.half[k] = d->cg_size[g2][k];
      const float* rf = reinterpret_cast<const float*>(&r);
      float* g = reinterpret_cast<float*>(reinterpret_cast<char*>(&d->pair_rec) + pair_tab_byte((unsigned)p));
      for (int k = 0; k < PAIR_REC / 4; k++)
        for (int c = 0; c < 4; c++) g[128 * k + c] = rf[4 * k + c];
    }
    {  // contact-side record
      PairCon& q = d->pair_con[p];
      memset(&q, 0, sizeof(q));
      q.sup = d->pair_sup[p];
      q.dm[0] = d->pair_dm[p][0];
      q.dm[1] = d->pair_dm[p][1];
      q.mu = d->pair_mu[p];
      q.tran = d->pair_tran[p];
      q.margin = d->pair_margin[p];
      q.b = d->pair_b[p];
      q.k = d->pair_k[p];
      for (int k = 0; k < 5; k++) q.solimp[k] = d->pair_solimp[p][k];
      // its first word group (sup, dm, mu) rides with the pair record: PairTab's seventh group
      memcpy(reinterpret_cast<char*>(&d->pair_rec) + pair_tab_byte((unsigned)p) + 512 * (PAIR_GROUPS - 1), &q, 16);
    }
    if (mm->cgeom_margin[g1] != 0 || mm->cgeom_margin[g2] != 0) return set_err(PP3_ERR_MODEL, "nonzero geom margins unsupported");
  }
  {  // sphere-box cull tables (DevModel::cull_on)
    d->cull_on = 0;
    d->cull_reach = 0.0f;
    memset(d->pair_box4, 0xFF, sizeof(d->pair_box4));
    memset(d->box_tab, 0, sizeof(d->box_tab));
    bool ok = d->nbox >= 1 && d->nbox <= 32 && d->npair > 32 && d->npair <= 32 * 5 && mm->body_parentid[1] == 0;
    const char* off = getenv("PP3_NO_CULL");  // tests only: every pair through the narrow phase
    if (off && off[0] == '1') ok = false;
    double reach = 0.0, margin = 0.0;
    for (int sl = 0; ok && sl < d->nrobot_geom; sl++) {  // chain of link offsets from body 1's origin
      const int g = d->robot_geom[sl];
      const double* gp = mm->cgeom_pos[g];
      double dist = sqrt(gp[0] * gp[0] + gp[1] * gp[1] + gp[2] * gp[2]);
      int b = mm->cgeom_bodyid[g];
      for (; b > 1; b = mm->body_parentid[b]) {
        const double* bp = mm->body_pos[b];
        dist += sqrt(bp[0] * bp[0] + bp[1] * bp[1] + bp[2] * bp[2]);
      }
      if (b != 1) ok = false;
      reach = fmax(reach, dist + mm->cgeom_size[g][0]);
    }
    for (int p = 0; ok && p < d->npair; p++) {
      const int g1 = mm->pair_g1[p], g2 = mm->pair_g2[p];
      const bool sb = mm->cgeom_type[g1] == PP3_GEOM_SPHERE && mm->cgeom_type[g2] == PP3_GEOM_BOX && box_slot[g2] >= 0;
      if (sb) margin = fmax(margin, (double)d->pair_margin[p]);
      if (p >= 32 && sb) {
        const int k = p / 32 - 1, ln = p % 32;
        d->pair_box4[ln] = (d->pair_box4[ln] & ~(0xFFu << (8 * k))) | ((uint32_t)box_slot[g2] << (8 * k));
      }
    }
    for (int g = 0; ok && g < mm->ncgeom; g++) {
      if (box_slot[g] < 0) continue;
      TerrainRec& t = d->box_tab[box_slot[g]];
      for (int k = 0; k < 3; k++) { t.p[k] = d->cg_pos[g][k]; t.half[k] = d->cg_size[g][k]; }
      for (int k = 0; k < 9; k++) t.R[k] = d->cg_wmat[g][k];
    }
    if (ok) {
      d->cull_reach = (float)(reach + margin + 0.01);
      d->cull_on = 1;
    }
  }
  d->nsite = mm->nsite;
  for (int s = 0; s < mm->nsite; s++) {
    d->site_body[s] = mm->site_bodyid[s];
    for (int k = 0; k < 3; k++) d->site_pos[s][k] = (float)mm->site_pos[s][k];
    for (int k = 0; k < 4; k++) d->site_quat[s][k] = (float)mm->site_quat[s][k];
  }
  if (mm->nsensor < 0 || mm->nsensor > PP3_MAX_SENSOR || mm->nsensordata > PP3_MAX_SENSORDATA)
    return set_err(PP3_ERR_MODEL, "too many sensors");
  d->nsensor = mm->nsensor;
  d->nsensordata = mm->nsensordata;
  for (int i = 0; i < mm->nsensor; i++) {
    d->sensor_type[i] = mm->sensor_type[i];
    d->sensor_objid[i] = mm->sensor_objid[i];
    d->sensor_adr[i] = mm->sensor_adr[i];
    d->sensor_cutoff[i] = (float)mm->sensor_cutoff[i];
    if (mm->sensor_objid[i] < 0 || mm->sensor_objid[i] >= mm->nsite) return set_err(PP3_ERR_MODEL, "sensor site id");
  }
  for (int b = 0; b < NB; b++) {
    d->body_parent[b] = mm->body_parentid[b];
    d->body_dofadr[b] = mm->body_dofadr[b];
    d->body_dofnum[b] = mm->body_dofnum[b];
  }
  for (int i = 0; i < mm->nsensor; i++) {  // the pipeline record's sensor lane records (fill_lane_records)
    int depth = 0;
    for (int bb = mm->site_bodyid[mm->sensor_objid[i]]; bb > 0; bb = mm->body_parentid[bb]) depth++;
    if (depth > LS_MAXCH) return set_err(PP3_ERR_MODEL, "sensor site body deeper than 4 levels");
  }
  for (int a = 0; a < NU; a++) {
    int j = mm->actuator_trnid[a];
    d->act_dof[a] = mm->jnt_dofadr[j];
    d->act_qadr[a] = mm->jnt_qposadr[j];
    if (mm->jnt_dofadr[j] != 6 + a) return set_err(PP3_ERR_MODEL, "actuator i must drive hinge dof 6+i");
    d->act_biastype[a] = mm->actuator_biastype[a];
    d->act_forcelimited[a] = mm->actuator_forcelimited[a];
    d->act_ctrllimited[a] = mm->actuator_ctrllimited[a];
    d->act_gear[a] = (float)mm->actuator_gear[a];
    d->act_gain[a] = (float)mm->actuator_gainprm[a][0];
    for (int k = 0; k < 3; k++) d->act_bias[a][k] = (float)mm->actuator_biasprm[a][k];
    for (int k = 0; k < 2; k++) {
      d->act_frange[a][k] = (float)mm->actuator_forcerange[a][k];
      d->act_crange[a][k] = (float)mm->actuator_ctrlrange[a][k];
    }
  }
  // environment
  d->n_frames = c->n_frames;
  d->H = c->obs_history;
  d->La = c->latency_len;
  d->Li = c->imu_latency_len;
  d->use_imu = c->use_imu;
  d->resample_step = c->resample_velocity_step;
  d->term_step = c->early_termination_step_threshold;
  d->torso_body = c->torso_body;
  if (c->torso_body < 1 || c->torso_body >= NB) return set_err(PP3_ERR_ARG, "torso body id out of range");
  for (int f = 0; f < 4; f++) {
    d->feet_site[f] = c->feet_site[f];
    d->lower_leg_body[f] = c->lower_leg_body[f];
    if (c->feet_site[f] < 0 || c->feet_site[f] >= mm->nsite) return set_err(PP3_ERR_ARG, "foot site not found");
    if (c->lower_leg_body[f] < 1 || c->lower_leg_body[f] >= NB) return set_err(PP3_ERR_ARG, "lower-leg body id out of range");
  }
  if (c->n_upper_leg_geoms < 0 || c->n_upper_leg_geoms > 16) return set_err(PP3_ERR_ARG, "n_upper_leg_geoms must be 0..16");
  if (c->n_torso_geoms < 0 || c->n_torso_geoms > 8) return set_err(PP3_ERR_ARG, "n_torso_geoms must be 0..8");
  d->n_knee_geoms = c->n_upper_leg_geoms;
  for (int i = 0; i < c->n_upper_leg_geoms && i < 16; i++) d->knee_geoms[i] = c->upper_leg_geoms[i];
  d->n_torso_geoms = c->n_torso_geoms;
  for (int i = 0; i < c->n_torso_geoms && i < 8; i++) d->torso_geoms[i] = c->torso_geoms[i];
  d->partitionable = c->rng_partitionable;
  d->imu_off = PP3_S_ACT_BUF + 12 * c->latency_len;
  d->stride = d->imu_off + 6 * c->imu_latency_len;
  for (int i = 0; i < PP3_MAX_LAG; i++) {
    d->lat_dist[i] = (float)c->latency_dist[i];
    d->imu_lat_dist[i] = (float)c->imu_latency_dist[i];
  }
  d->action_scale = (float)c->action_scale;
  for (int j = 0; j < NU; j++) {
    d->default_pose[j] = (float)c->default_pose[j];
    d->jlo[j] = (float)c->joint_lower[j];
    d->jhi[j] = (float)c->joint_upper[j];
  }
  for (int k = 0; k < 4; k++) d->des_abd[k] = (float)c->desired_abduction[k];
  for (int k = 0; k < 3; k++) {
    d->start_lo[k] = (float)c->start_pos_min[k];
    d->start_hi[k] = (float)c->start_pos_max[k];
    d->des_z[k] = (float)c->desired_world_z[k];
  }
  for (int k = 0; k < 2; k++) {
    d->cmd_x[k] = (float)c->lin_vel_x_range[k];
    d->cmd_y[k] = (float)c->lin_vel_y_range[k];
    d->cmd_w[k] = (float)c->ang_vel_range[k];
  }
  d->zero_cmd_p = (float)c->zero_command_probability;
  d->stand_thr = (float)c->stand_still_command_threshold;
  d->max_pitch = (float)c->max_pitch_command;
  d->max_roll = (float)c->max_roll_command;
  d->n_ang = (float)c->ang_vel_noise;
  d->n_grav = (float)c->gravity_noise;
  d->n_motor = (float)c->motor_angle_noise;
  d->n_act = (float)c->last_action_noise;
  d->kick_vel = (float)c->kick_vel;
  d->kick_p = (float)c->kick_probability;
  d->term_z = (float)c->terminal_body_z;
  d->cos_term_angle = (float)cos(c->terminal_body_angle);
  d->foot_radius = (float)c->foot_radius;
  d->env_dt = (float)c->env_dt;
  d->dt = (float)c->dt;
  for (int k = 0; k < PP3_NREWARD; k++) d->scales[k] = (float)c->reward_scales[k];
  d->sigma = (float)c->tracking_sigma;
  d->pi_f = 3.14159265358979323846f;
  fill_lane_records(d);
  return PP3_OK;
}
