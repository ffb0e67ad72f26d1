// gpd_dcontact.h — the drone <-> drone contact of one-wave blocks (DcLds ... DcHookT): its LDS
// layout, the block's pair table, broadphase, contact rows, the island's plane rows and the
// projected Gauss-Seidel solve (dc_solve), and the hook bullet_substep calls every substep.
// Needs the narrowphase (gpd_narrowphase.h), SimView and wave_lds_sync (gpd_layout.h) and the
// plane solve's row rules (gpd_device.h).
#pragma once
#include "gpd_narrowphase.h"

namespace gpd {

enum { DC_CX, DC_CY, DC_CZ, DC_AX, DC_AY, DC_AZ, DC_PX, DC_PY, DC_PZ, DC_VX, DC_VY, DC_VZ, DC_WX, DC_WY, DC_WZ,
       DC_I00, DC_I01, DC_I02, DC_I11, DC_I12, DC_I22, DC_DLX, DC_DLY, DC_DLZ, DC_DAX, DC_DAY, DC_DAZ,
       DC_R0, DC_R1, DC_R3, DC_R4, DC_R6, DC_R7, DC_N };   // DC_R*: the basis entries beside the axis (Rm[2,5,8])
constexpr int kDcChunks = 32;   // pair chunks of a block: <= 64 (D-1) / 2 / 64 + 1 for D <= 64
constexpr int kDcPts = 4;       // contacts per pair: Bullet's MANIFOLD_CACHE_SIZE (bullet_mb.pair_manifold)
constexpr int kDcConPasses = kDcPts * kDcChunks;   // 64-contact passes of a block
// a near pair's narrowphase, staged for the lanes that set up its contacts' rows
enum { DS_N = 0, DS_PB = 3, DS_D = 6, DS_FP = 7, DS_FD = 19, DS_NUM = 23 };
// an island drone's plane rows (bullet_mb._plane_rows_world): world arms, rhs, 1/jacDiag, jacDiag, impulses
enum { DI_RW = 0, DI_RHS = 12, DI_JDI = 24, DI_JDN = 36, DI_LAM = 40, DI_NUM = 52 };
template <typename R>
struct DcLds {
  R dc[DC_N][kWave];                  // drone columns
  // one area, three uses at different times: a pass's narrowphases (st: normal, point, distance,
  // face points per near slot; rim: per near slot and rim the best start's (x, y) and whether the
  // rim is needed), then, after the last pass, the island drones' plane rows (isl)
  R u[DI_NUM][kWave];
  unsigned long long nearw[kDcChunks], contw[kDcConPasses];   // pairs in reach (by chunk) / contacts (by pass)
  R eres[kWave];                      // per env: this iteration's largest squared residual
  int edone[kWave];                   // per env: solve finished
  int stouch[kWave];                  // drone in a contact
  int island[kWave];                  // drone whose plane rows the solve takes (its own plane solve skipped)
  int cij[kWave], clev[kWave];        // contacts 0..63: the lane's contact (i | j << 8) and its level
  int cij1[kWave], clev1[kWave];      // contacts 64..127 (the lanes' second register row)
  int dlev[kWave];                    // per drone: the level of its last contact (level pass)
  int nsp[kWave], nsij[kWave];        // this pass's near pairs: pair index, i | j << 8
  int qmap[kDcPts * kWave];           // this pass's contacts: near slot | point << 8 (0 closest, 1..4 face)
  int npdone[kWave];                  // narrowphase: near slot resolved at an earlier margin level
  int ecnt[kWave], ek0[kWave], ek1[kWave];   // per env: contacts, their contact-index range [ek0, ek1)
};
// The Gauss-Seidel sweeps' staging (the compiled-in PYB flag-set kernels, STAGE = true; the
// run-time-flag kernels, which serve the long observation tiles, recompute instead): operands that
// do not change over a solve's iterations, formed once at the setup - the same operations on the
// same operands as the recomputation, so the same bits.
//   ig: an island drone's plane points: the inverse-inertia images of the angular Jacobians, per
//       point p: normal G (3 p ..), friction along (0,-1,0) H, along (1,0,0) K;
//   pj: a first register row's (contacts 0..63) angular Jacobians and images per direction q (n,
//       t1, t2): pj[12 q + x][contact], x = A 0..2 (r_A x d), B 3..5 (r_B x d), gA 6..8, gB 9..11.
enum { DG_G = 0, DG_H = 12, DG_K = 24, DG_NUM = 36 };
constexpr int kPj = 36;
template <typename R>
struct DcStage {
  R ig[DG_NUM][kWave];
  R pj[kPj][kWave];
};
template <typename R>
__device__ __forceinline__ DcStage<R>& dc_stage() {
  __shared__ DcStage<R> x;
  return x;
}
static_assert(DS_NUM + 4 * 7 <= DI_NUM, "narrowphase staging fits the island rows' area");
#define DC_ST(k) u[k]
#define DC_RIM(m, e) u[DS_NUM + 7 * (m) + (e)]
#define DC_ISL(k) u[k]
// one LDS block per instantiation, shared by the hook (inlined) and the solve (a call)
template <typename R>
__device__ __forceinline__ DcLds<R>& dc_lds() {
  __shared__ DcLds<R> x;
  return x;
}
// the per-block layout a kernel hands to the hook (its prologue computes it once)
struct DcPairs {
  int npairs, P, D, nch;   // pairs of the block's whole envs, per env, drones per env, chunks
  int pij[4];              // chunks 0..3: this lane's pair as (lane i) | (lane j) << 8, -1 = none
  int pmagic;              // p / P == (p * pmagic) >> 24 for p < npairs (host-checked)
  const int* tab;          // [P] pair q -> i | j << 8 (env-local drones), for chunks >= 4
  void* rows;              // this block's row store (chunks >= 1), or null
};
__device__ __forceinline__ DcPairs dc_pairs_none() {
  DcPairs dp;
  dp.npairs = dp.P = dp.nch = dp.pmagic = 0;
  dp.D = 1;
  dp.pij[0] = dp.pij[1] = dp.pij[2] = dp.pij[3] = -1;
  dp.tab = nullptr;
  dp.rows = nullptr;
  return dp;
}
// whether a kernel of flag set PF runs the drone <-> drone contact (multi-drone PYB* envs)
template <bool MULTI, int PF>
__device__ __forceinline__ bool dc_enabled(int flags) {
  return MULTI && pf_on<PF>(flags, F_BULLET) && !pf_on<PF>(flags, F_NO_DC);
}
__device__ __forceinline__ int dc_pair_lanes(const DcPairs& dp, int p);
// this lane's pair of chunk ch (registers for chunks 0..3, selects rather than a dynamic index)
__device__ __forceinline__ int dc_pair_of(const DcPairs& dp, int ch, int p) {
  if (ch >= 4) return dc_pair_lanes(dp, p);
  return ch == 0 ? dp.pij[0] : (ch == 1 ? dp.pij[1] : (ch == 2 ? dp.pij[2] : dp.pij[3]));
}
__device__ __forceinline__ int dc_pair_lanes(const DcPairs& dp, int p) {
  const int e = (p * dp.pmagic) >> 24;
  const int t = dp.tab[p - e * dp.P];
  return ((t & 255) + e * dp.D) | (((t >> 8) + e * dp.D) << 8);
}
template <typename R>
__device__ __forceinline__ DcPairs dc_pairs_for(const SimView<R>& v, int tid, int nact) {
  DcPairs dp;
  dp.P = v.dcP;
  dp.D = v.D;
  dp.npairs = v.dcP > 0 ? (nact / v.D) * v.dcP : 0;
  dp.nch = (dp.npairs + kWave - 1) / kWave;
  dp.pmagic = v.dc_pmagic;
  dp.tab = v.dc_tab;
  dp.rows = v.dc_rows ? (void*)((R*)v.dc_rows + (long long)blockIdx.x * v.dc_row_stride) : nullptr;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    const int p = tid + kWave * ch;
    dp.pij[ch] = p < dp.npairs ? dc_pair_lanes(dp, p) : -1;
  }
  return dp;
}
// broadphase of the pair (i, j) (oracle/bullet_mb.py pair_near): the sphere test, then the
// separating-axis rejects; the centre / axis columns written
template <typename R>
__device__ __forceinline__ bool dc_near(const DcLds<R>& L, int i, int j, const Consts<R>& c) {
  const R ex = L.dc[DC_CX][i] - L.dc[DC_CX][j], ey = L.dc[DC_CY][i] - L.dc[DC_CY][j],
          ez = L.dc[DC_CZ][i] - L.dc[DC_CZ][j];
  const R e2 = pc_dot(ex, ey, ez, ex, ey, ez);
  if (GPD_RARE(e2 < c.dd_reach2)) {
    const R ax = L.dc[DC_AX][i], ay = L.dc[DC_AY][i], az = L.dc[DC_AZ][i];
    const R bx = L.dc[DC_AX][j], by = L.dc[DC_AY][j], bz = L.dc[DC_AZ][j];
    const R r = c.cyl_r, hh = c.cyl_hh, lim = c.brk + R(1e-9);
    const R tilt = cyl_extent_cos(pc_dot(ax, ay, az, bx, by, bz), r, hh);   // one along the other's axis
    const R ea = pc_dot(ex, ey, ez, ax, ay, az), eb = pc_dot(ex, ey, ez, bx, by, bz);
    if (g_abs(ea) - (hh + tilt) > lim) return false;
    if (g_abs(eb) - (hh + tilt) > lim) return false;
    if (e2 > R(0)) {
      const R l = g_sqrt(e2);
      const R ext = cyl_extent_cos(ea / l, r, hh) + cyl_extent_cos(eb / l, r, hh);
      if (l - ext > lim) return false;
    }
    return true;
  }
  return false;
}
// a contact's rows: directions (n, t1, t2), the arms of A (= i) and B (= j) from their COMs, rhs,
// 1/jacDiag, the normal row's jacDiag, impulses - 25 reals (the angular Jacobians r x d and their
// I_w^-1 images are formed at each use from the arms and the drones' inverse inertias, the same
// operations as at the setup, so the values are the same bit for bit)
template <typename R>
struct DcRow {
  R d[3][3], ra[3], rb[3], rhs[3], jdi[3], jdn, lam[3];
  int i, j, env, rank;
};
constexpr int kRowReal = 25, kRowLam = 22;   // reals of a row; offset of lam
// the world inverse inertias (symmetric: 00 01 02 11 12 22) of a row's two drones
template <typename R>
struct DcInv {
  R a[6], b[6];
};
template <typename R>
__device__ __forceinline__ void dc_inv(const DcLds<R>& L, int i, int j, DcInv<R>& I) {
#pragma unroll
  for (int x = 0; x < 6; ++x) { I.a[x] = L.dc[DC_I00 + x][i]; I.b[x] = L.dc[DC_I00 + x][j]; }
}
template <typename R>
__device__ __forceinline__ void dc_cross(const R r[3], const R d[3], R o[3]) {
  o[0] = r[1] * d[2] - r[2] * d[1]; o[1] = r[2] * d[0] - r[0] * d[2]; o[2] = r[0] * d[1] - r[1] * d[0];
}
template <typename R>
__device__ __forceinline__ void dc_symv(const R m[6], const R v[3], R o[3]) {
  o[0] = pc_dot(m[0], m[1], m[2], v[0], v[1], v[2]);
  o[1] = pc_dot(m[1], m[3], m[4], v[0], v[1], v[2]);
  o[2] = pc_dot(m[2], m[4], m[5], v[0], v[1], v[2]);
}
template <bool STAGE, typename R>
__device__ __forceinline__ void dc_row_setup(const DcLds<R>& L, int i, int j, const R n[3], const R pb[3], R dist,
                                             const Consts<R>& c, R inv_m, R idt, DcRow<R>& w, int slot) {
  const R pa[3] = {pb[0] + n[0] * dist, pb[1] + n[1] * dist, pb[2] + n[2] * dist};
  w.ra[0] = pa[0] - L.dc[DC_PX][i]; w.ra[1] = pa[1] - L.dc[DC_PY][i]; w.ra[2] = pa[2] - L.dc[DC_PZ][i];
  w.rb[0] = pb[0] - L.dc[DC_PX][j]; w.rb[1] = pb[1] - L.dc[DC_PY][j]; w.rb[2] = pb[2] - L.dc[DC_PZ][j];
  R t1[3], t2[3];
  plane_space(n, t1, t2);
  DcInv<R> I;
  dc_inv(L, i, j, I);
  const R dvx = L.dc[DC_VX][i] - L.dc[DC_VX][j], dvy = L.dc[DC_VY][i] - L.dc[DC_VY][j], dvz = L.dc[DC_VZ][i] - L.dc[DC_VZ][j];
  const R wa[3] = {L.dc[DC_WX][i], L.dc[DC_WY][i], L.dc[DC_WZ][i]};
  const R wb[3] = {L.dc[DC_WX][j], L.dc[DC_WY][j], L.dc[DC_WZ][j]};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const R* d = q == 0 ? n : (q == 1 ? t1 : t2);
    w.d[q][0] = d[0]; w.d[q][1] = d[1]; w.d[q][2] = d[2];
    R A[3], B[3], gA[3], gB[3];
    dc_cross(w.ra, d, A);
    dc_cross(w.rb, d, B);
    dc_symv(I.a, A, gA);
    dc_symv(I.b, B, gB);
    if (STAGE && slot >= 0) {   // a first register row: the sweeps read these instead of recomputing them
      DcStage<R>& G = dc_stage<R>();
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        G.pj[12 * q + e][slot] = A[e]; G.pj[12 * q + 3 + e][slot] = B[e];
        G.pj[12 * q + 6 + e][slot] = gA[e]; G.pj[12 * q + 9 + e][slot] = gB[e];
      }
    }
    const R jd = (inv_m + inv_m + pc_dot(A[0], A[1], A[2], gA[0], gA[1], gA[2])) + pc_dot(B[0], B[1], B[2], gB[0], gB[1], gB[2]);
    const R rel = (pc_dot(d[0], d[1], d[2], dvx, dvy, dvz) + pc_dot(A[0], A[1], A[2], wa[0], wa[1], wa[2])) -
                  pc_dot(B[0], B[1], B[2], wb[0], wb[1], wb[2]);
    // 1/jd and x/dt as Newton-refined reciprocals (jd >= 2/m > 0): ~1 ulp from the quotients
    const R inv = g_rcp(jd);
    if (q == 0) {
      const R pen = dist + c.slop;
      w.rhs[0] = pen > R(0) ? (-rel - pen * idt) * inv : (-pen * c.erp * idt - rel) * inv;
      w.jdn = jd;
    } else {
      w.rhs[q] = -rel * inv;
    }
    w.jdi[q] = inv;
    w.lam[q] = R(0);
  }
  w.i = i;
  w.j = j;
}
// a row's angular Jacobians A = r_A x d_q, B = r_B x d_q and their images I_A^-1 A, I_B^-1 B: recomputed
// from the arms and the drones' inverse inertias (rows in the row store), or read from the setup's
// staging (register rows, L.pj) - the same operations on the same operands, so the same bits
template <typename R>
struct DcJacRow {
  const DcRow<R>& w;
  const DcInv<R>& I;
  __device__ __forceinline__ void operator()(int q, R A[3], R B[3], R gA[3], R gB[3]) const {
    dc_cross(w.ra, w.d[q], A);
    dc_cross(w.rb, w.d[q], B);
    dc_symv(I.a, A, gA);
    dc_symv(I.b, B, gB);
  }
};
template <typename R>
struct DcJacLds {
  const DcStage<R>& G;
  int slot;
  __device__ __forceinline__ void operator()(int q, R A[3], R B[3], R gA[3], R gB[3]) const {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      A[e] = G.pj[12 * q + e][slot]; B[e] = G.pj[12 * q + 3 + e][slot];
      gA[e] = G.pj[12 * q + 6 + e][slot]; gB[e] = G.pj[12 * q + 9 + e][slot];
    }
  }
};
// the rows' Jacobian products and impulse application (vi / vj: the two drones' deltas, linear
// then angular)
template <typename R>
__device__ __forceinline__ R dc_jv(const DcRow<R>& w, int q, const R A[3], const R B[3], const R vi[6], const R vj[6]) {
  return (pc_dot(w.d[q][0], w.d[q][1], w.d[q][2], vi[0] - vj[0], vi[1] - vj[1], vi[2] - vj[2]) +
          pc_dot(A[0], A[1], A[2], vi[3], vi[4], vi[5])) -
         pc_dot(B[0], B[1], B[2], vj[3], vj[4], vj[5]);
}
template <typename R>
__device__ __forceinline__ void dc_apply(const DcRow<R>& w, int q, R delta, R inv_m, const R gA[3], const R gB[3], R vi[6],
                                         R vj[6]) {
  const R dm = inv_m * delta;
  vi[0] = vi[0] + w.d[q][0] * dm; vi[1] = vi[1] + w.d[q][1] * dm; vi[2] = vi[2] + w.d[q][2] * dm;
  vi[3] = vi[3] + gA[0] * delta; vi[4] = vi[4] + gA[1] * delta; vi[5] = vi[5] + gA[2] * delta;
  vj[0] = vj[0] - w.d[q][0] * dm; vj[1] = vj[1] - w.d[q][1] * dm; vj[2] = vj[2] - w.d[q][2] * dm;
  vj[3] = vj[3] - gB[0] * delta; vj[4] = vj[4] - gB[1] * delta; vj[5] = vj[5] - gB[2] * delta;
}
// one normal row (bullet_mb.drone_contact's normal loop); returns the row's squared residual
template <typename R, typename J>
__device__ __forceinline__ R dc_normal(DcRow<R>& w, R inv_m, R vi[6], R vj[6], const J& jac) {
  R A[3], B[3], gA[3], gB[3];
  jac(0, A, B, gA, gB);
  R delta = w.rhs[0] - w.jdi[0] * dc_jv(w, 0, A, B, vi, vj);
  const R sum = w.lam[0] + delta;
  const bool neg = sum < R(0);
  delta = neg ? -w.lam[0] : delta;
  w.lam[0] = neg ? R(0) : sum;
  dc_apply(w, 0, delta, inv_m, gA, gB, vi, vj);
  const R rr = delta * w.jdn;
  return rr * rr;
}
// one friction pair on the cone (only while the normal impulse is positive); squared residual
template <typename R, typename J>
__device__ __forceinline__ R dc_friction(DcRow<R>& w, R mu, R inv_m, R vi[6], R vj[6], const J& jac) {
  if (!(w.lam[0] > R(0))) return R(0);
  R A1[3], B1[3], gA1[3], gB1[3], A2[3], B2[3], gA2[3], gB2[3];
  jac(1, A1, B1, gA1, gB1);
  jac(2, A2, B2, gA2, gB2);
  const R lim = mu * w.lam[0];
  R s1 = w.lam[1] + (w.rhs[1] - w.jdi[1] * dc_jv(w, 1, A1, B1, vi, vj));
  R s2 = w.lam[2] + (w.rhs[2] - w.jdi[2] * dc_jv(w, 2, A2, B2, vi, vj));
  const R m2 = s1 * s1 + s2 * s2;
  if (m2 > lim * lim) {
    const R f = lim * g_rsqrt1(m2);   // one Newton step: ~1e-14 relative on the projected impulse
    s1 = s1 * f;
    s2 = s2 * f;
  }
  const R e1 = s1 - w.lam[1], e2 = s2 - w.lam[2];
  w.lam[1] = s1;
  w.lam[2] = s2;
  dc_apply(w, 1, e1, inv_m, gA1, gB1, vi, vj);
  dc_apply(w, 2, e2, inv_m, gA2, gB2, vi, vj);
  const R rr = e1 + e2;
  return rr * rr;
}
// the row store: per chunk, element x of lane ln at chunk[x * 64 + ln] (kRowReal reals), then the
// four ints (i, j, env, rank) at ints[k * 64 + ln] behind them
template <typename R>
__device__ __forceinline__ void dc_row_store(R* chunk, int ln, const DcRow<R>& w) {
  const R* src = &w.d[0][0];
#pragma unroll
  for (int x = 0; x < kRowReal; ++x) chunk[x * kWave + ln] = src[x];
  int* di = reinterpret_cast<int*>(chunk + kRowReal * kWave);
  di[ln] = w.i; di[kWave + ln] = w.j; di[2 * kWave + ln] = w.env; di[3 * kWave + ln] = w.rank;
}
template <typename R>
__device__ __forceinline__ void dc_row_load(const R* chunk, int ln, DcRow<R>& w) {
  R* dst = &w.d[0][0];
#pragma unroll
  for (int x = 0; x < kRowReal; ++x) dst[x] = chunk[x * kWave + ln];
  const int* si = reinterpret_cast<const int*>(chunk + kRowReal * kWave);
  w.i = si[ln]; w.j = si[kWave + ln]; w.env = si[2 * kWave + ln]; w.rank = si[3 * kWave + ln];
}
// R elements of one row in the store: kRowReal reals + 4 ints, column-major over the chunk's 64 lanes
template <typename R>
__host__ __device__ constexpr int dc_row_reals() { return kRowReal + (4 * 4 + (int)sizeof(R) - 1) / (int)sizeof(R); }
constexpr int kDcRegRows = 2;   // contacts 0..127 of a block in the lanes' registers (two rows a lane)

// the setup and solve: a call, so that its registers stay out of the substep loop that almost
// never enters it (the caller parks its own values in LDS around it: bullet_substep).  Inlined at
// each substep call site it measured slower (profiles/r3/dc/ab_inline.log, profiles/r4/dc_call/).
// wave-wide exclusive prefix sum of small non-negative ints (and the total)
__device__ __forceinline__ int wave_excl_scan(int x, int ln, int& total) {
  int v = x;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int y = __shfl_up(v, o);
    if (ln >= o) v += y;
  }
  total = __shfl(v, kWave - 1);
  return v - x;
}
// an island drone's plane rows (bullet_mb._plane_rows_world; plane_contact_regs' world form): lane ln's
// columns of L.isl; returns whether any of its four points is active
template <bool STAGE, typename R>
__device__ __forceinline__ bool island_rows(DcLds<R>& L, int ln, const Consts<R>& c, R inv_m, R idt) {
  const R Rm[9] = {L.dc[DC_R0][ln], L.dc[DC_R1][ln], L.dc[DC_AX][ln], L.dc[DC_R3][ln], L.dc[DC_R4][ln],
                   L.dc[DC_AY][ln], L.dc[DC_R6][ln], L.dc[DC_R7][ln], L.dc[DC_AZ][ln]};
  const R i00 = L.dc[DC_I00][ln], i01 = L.dc[DC_I01][ln], i02 = L.dc[DC_I02][ln], i11 = L.dc[DC_I11][ln],
          i12 = L.dc[DC_I12][ln], i22 = L.dc[DC_I22][ln];
  const R px = L.dc[DC_PX][ln], py = L.dc[DC_PY][ln], pz = L.dc[DC_PZ][ln];
  const R vx = L.dc[DC_VX][ln], vy = L.dc[DC_VY][ln], vz = L.dc[DC_VZ][ln];
  const R wx = L.dc[DC_WX][ln], wy = L.dc[DC_WY][ln], wz = L.dc[DC_WZ][ln];
  const R zc = (-Rm[8] < R(0) ? -c.cyl_hh : c.cyl_hh) + c.cyl_zoff;
  const R cr = c.cyl_r;
  bool any = false;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const R rx = p == 0 ? cr : (p == 2 ? -cr : R(0)), ry = p == 1 ? cr : (p == 3 ? -cr : R(0));
    const R rwx = pc_dot(Rm[0], Rm[1], Rm[2], rx, ry, zc);
    const R rwy = pc_dot(Rm[3], Rm[4], Rm[5], rx, ry, zc);
    const R rwz = pc_dot(Rm[6], Rm[7], Rm[8], rx, ry, zc);
    L.DC_ISL(DI_RW + 3 * p)[ln] = rwx; L.DC_ISL(DI_RW + 3 * p + 1)[ln] = rwy; L.DC_ISL(DI_RW + 3 * p + 2)[ln] = rwz;
    const R dist = pz + rwz;
    const bool act = dist < c.brk && g_abs(px + rwx) <= c.plane_half && g_abs(py + rwy) <= c.plane_half;
    any = any || act;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const R ax = j == 0 ? rwy : (j == 1 ? rwz : R(0));
      const R ay = j == 0 ? -rwx : (j == 1 ? R(0) : rwz);
      const R az = j == 0 ? R(0) : (j == 1 ? -rwx : -rwy);
      const R gx = pc_dot(i00, i01, i02, ax, ay, az), gy = pc_dot(i01, i11, i12, ax, ay, az),
              gz = pc_dot(i02, i12, i22, ax, ay, az);
      if (STAGE) {
        DcStage<R>& G = dc_stage<R>();
        const int gk = (j == 0 ? DG_G : (j == 1 ? DG_H : DG_K)) + 3 * p;
        G.ig[gk][ln] = gx; G.ig[gk + 1][ln] = gy; G.ig[gk + 2][ln] = gz;
      }
      const R jd = inv_m + pc_dot(ax, ay, az, gx, gy, gz);
      const R inv = g_rcp(jd);
      const R vl = j == 0 ? vz : (j == 1 ? -vy : vx);
      const R rel = vl + pc_dot(ax, ay, az, wx, wy, wz);
      R r;
      if (j == 0) {
        const R pen = dist + c.slop;
        r = pen > R(0) ? (-rel - pen * idt) * inv : (-pen * c.erp * idt - rel) * inv;
        L.DC_ISL(DI_JDN + p)[ln] = act ? jd : R(0);
      } else {
        r = -rel * inv;
      }
      L.DC_ISL(DI_JDI + 3 * p + j)[ln] = act ? inv : R(0);
      L.DC_ISL(DI_RHS + 3 * p + j)[ln] = act ? r : R(0);
      L.DC_ISL(DI_LAM + 3 * p + j)[ln] = R(0);
    }
  }
  return any;
}
// one sweep of an island drone's plane rows (normal rows or friction pairs) on its LDS deltas;
// returns the largest squared residual.  Branch-free: every operand is loaded before the chain
// starts, and a point the oracle skips (inactive: no row; a friction pair whose normal impulse is
// not positive) takes a zero step - the same values bit for bit (x + 0 * y == x for finite y).
template <bool STAGE, typename R>
__device__ __forceinline__ R island_sweep(DcLds<R>& L, int ln, bool friction, R mu, R inv_m) {
  const DcStage<R>& G = dc_stage<R>();
  R dl0 = L.dc[DC_DLX][ln], dl1 = L.dc[DC_DLY][ln], dl2 = L.dc[DC_DLZ][ln];
  R da0 = L.dc[DC_DAX][ln], da1 = L.dc[DC_DAY][ln], da2 = L.dc[DC_DAZ][ln];
  const R i00 = L.dc[DC_I00][ln], i01 = L.dc[DC_I01][ln], i02 = L.dc[DC_I02][ln], i11 = L.dc[DC_I11][ln],
          i12 = L.dc[DC_I12][ln], i22 = L.dc[DC_I22][ln];
  R rw[4][3], lam[4][3], rhs[4][3], jdi[4][3], jdn[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      rw[p][e] = L.DC_ISL(DI_RW + 3 * p + e)[ln];
      lam[p][e] = L.DC_ISL(DI_LAM + 3 * p + e)[ln];
      rhs[p][e] = L.DC_ISL(DI_RHS + 3 * p + e)[ln];
      jdi[p][e] = L.DC_ISL(DI_JDI + 3 * p + e)[ln];
    }
    jdn[p] = L.DC_ISL(DI_JDN + p)[ln];
  }
  R res = R(0);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    // a point no island lane of the wave has a row for (inactive, or a friction pair whose normal
    // impulse is not positive) is skipped by the whole wave: its zero step changes nothing
    if (__ballot(friction ? lam[p][0] > R(0) : jdn[p] > R(0)) == 0ull) continue;
    const R rwx = rw[p][0], rwy = rw[p][1], rwz = rw[p][2];
    if (!friction) {
      // an inactive point has rhs = jdi = jdn = 0 and lam = 0: delta = 0
      const R ax = rwy, ay = -rwx;
      const R g0 = STAGE ? G.ig[DG_G + 3 * p][ln] : pc_dot(i00, i01, i02, ax, ay, R(0));
      const R g1 = STAGE ? G.ig[DG_G + 3 * p + 1][ln] : pc_dot(i01, i11, i12, ax, ay, R(0));
      const R g2 = STAGE ? G.ig[DG_G + 3 * p + 2][ln] : pc_dot(i02, i12, i22, ax, ay, R(0));
      const R jv = dl2 + (ax * da0 + ay * da1);
      R delta = rhs[p][0] - jdi[p][0] * jv;
      const R sum = lam[p][0] + delta;
      const bool neg = sum < R(0);
      delta = neg ? -lam[p][0] : delta;
      lam[p][0] = neg ? R(0) : sum;
      dl2 = dl2 + inv_m * delta;
      da0 = da0 + g0 * delta;
      da1 = da1 + g1 * delta;
      da2 = da2 + g2 * delta;
      const R rr = delta * jdn[p];
      res = g_fmax(res, rr * rr);
    } else {
      const R lnrm = lam[p][0];
      const bool act = lnrm > R(0);
      const R lim = mu * lnrm;
      const R l1 = lam[p][1], l2 = lam[p][2];
      // (0,-1,0): a = (rz, 0, -rx); (1,0,0): a = (0, rz, -ry)
      const R h0 = STAGE ? G.ig[DG_H + 3 * p][ln] : pc_dot(i00, i01, i02, rwz, R(0), -rwx);
      const R h1 = STAGE ? G.ig[DG_H + 3 * p + 1][ln] : pc_dot(i01, i11, i12, rwz, R(0), -rwx);
      const R h2 = STAGE ? G.ig[DG_H + 3 * p + 2][ln] : pc_dot(i02, i12, i22, rwz, R(0), -rwx);
      const R k0 = STAGE ? G.ig[DG_K + 3 * p][ln] : pc_dot(i00, i01, i02, R(0), rwz, -rwy);
      const R k1 = STAGE ? G.ig[DG_K + 3 * p + 1][ln] : pc_dot(i01, i11, i12, R(0), rwz, -rwy);
      const R k2 = STAGE ? G.ig[DG_K + 3 * p + 2][ln] : pc_dot(i02, i12, i22, R(0), rwz, -rwy);
      const R j1 = (rwz * da0 - rwx * da2) - dl1;
      const R j2 = (rwz * da1 - rwy * da2) + dl0;
      R s1 = l1 + (rhs[p][1] - jdi[p][1] * j1);
      R s2 = l2 + (rhs[p][2] - jdi[p][2] * j2);
      const R m2 = s1 * s1 + s2 * s2;
      const bool cap = m2 > lim * lim;
      const R f = cap ? lim * g_rsqrt1(cap ? m2 : R(1)) : R(1);
      s1 = s1 * f;
      s2 = s2 * f;
      const R d1 = act ? s1 - l1 : R(0), d2 = act ? s2 - l2 : R(0);
      lam[p][1] = act ? s1 : l1;
      lam[p][2] = act ? s2 : l2;
      dl1 = dl1 - inv_m * d1;
      dl0 = dl0 + inv_m * d2;
      da0 = da0 + h0 * d1;
      da1 = da1 + h1 * d1;
      da2 = da2 + h2 * d1;
      da0 = da0 + k0 * d2;
      da1 = da1 + k1 * d2;
      da2 = da2 + k2 * d2;
      const R rr = d1 + d2;
      res = g_fmax(res, rr * rr);
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (!friction) {
      L.DC_ISL(DI_LAM + 3 * p)[ln] = lam[p][0];
    } else {
      L.DC_ISL(DI_LAM + 3 * p + 1)[ln] = lam[p][1];
      L.DC_ISL(DI_LAM + 3 * p + 2)[ln] = lam[p][2];
    }
  }
  L.dc[DC_DLX][ln] = dl0; L.dc[DC_DLY][ln] = dl1; L.dc[DC_DLZ][ln] = dl2;
  L.dc[DC_DAX][ln] = da0; L.dc[DC_DAY][ln] = da1; L.dc[DC_DAZ][ln] = da2;
  return res;
}
template <typename R>
__device__ __forceinline__ void eres_max(DcLds<R>& L, int env, R rr) {
  // the max through an LDS atomic on the bit pattern (non-negative floats order as unsigned integers)
  if (sizeof(R) == 8)
    atomicMax(reinterpret_cast<unsigned long long*>(&L.eres[env]), (unsigned long long)__double_as_longlong((double)rr));
  else
    atomicMax(reinterpret_cast<unsigned int*>(&L.eres[env]), (unsigned int)__float_as_uint((float)rr));
}
// The narrowphases of a pass's nthis near pairs (L.nsij[0..nthis)): bullet_mb.pair_geometry per pair,
// its 4 x 16 rim Newton chains as 64 tasks over the lanes (task t: slot t / 64, rim (t / 16) % 4,
// start t % 16; the best start per rim by a butterfly over 16 lanes, ties to the lower start), the
// closed-form candidates and the selection by the pair's own lane (lane = slot), margin level by
// margin level while some pair's cores overlap; then the fallback and the face manifold.  Lane
// ln < nthis stages its pair's result in L.st and its face-point mask in L.nsp[ln] and returns its
// contact count.  dc_narrow_pass: a call, so its registers stay out of dc_solve's Gauss-Seidel
// loops; dc_solve_body<.., INL = true> inlines it (see DcHookT).
template <typename R>
__device__ __forceinline__ int dc_narrow_pass_body(const Consts<R>* cp, int ln, int nthis) {
  DcLds<R>& L = dc_lds<R>();
  const Consts<R>& c = *cp;
#ifdef GPD_CONTACT_STATS
  unsigned long long tn0 = __builtin_readcyclecounter(), tn_task = 0, tn_sel = 0;
#endif
  const R margins[4] = {R(0.001), R(0.003), R(0.006), R(0.011)};
  const bool mine = ln < nthis;
  const int pij = mine ? L.nsij[ln] : 0;
  const int mi = pij & 255, mj = pij >> 8;
  const R ca[3] = {L.dc[DC_CX][mi], L.dc[DC_CY][mi], L.dc[DC_CZ][mi]}, aa[3] = {L.dc[DC_AX][mi], L.dc[DC_AY][mi], L.dc[DC_AZ][mi]};
  const R cb[3] = {L.dc[DC_CX][mj], L.dc[DC_CY][mj], L.dc[DC_CZ][mj]}, ab[3] = {L.dc[DC_AX][mj], L.dc[DC_AY][mj], L.dc[DC_AZ][mj]};
  NpPair<R> own;
  np_pair(ca, aa, cb, ab, own);
  bool found = !mine;
  R n[3] = {R(0), R(0), R(1)}, pb[3] = {R(0), R(0), R(0)}, dist = R(0), mgf = R(-1);
  R yl[3] = {R(0), R(0), R(0)};
  L.npdone[ln] = found ? 1 : 0;
  wave_lds_sync();
  const int ntask = nthis * 64;
#pragma unroll 1
  for (int lv = 0; lv < 4; ++lv) {
    if (__ballot(!found) == 0ull) break;
    const R mg = margins[lv], r = c.cyl_r - mg, h = c.cyl_hh - mg;
#pragma unroll 1
    for (int t0 = 0; t0 < ntask; t0 += kWave) {
      const int t = t0 + ln;
      // task t: slot t / 64, rim (t / 16) % 4, start t % 16 (bullet_mb.RIM_STARTS)
      const int slot = (t >> 6) & 63, rim = (t >> 4) & 3, k = t & 15;
      R f = R(INFINITY), x[3] = {R(0), R(0), R(0)}, y[3] = {R(0), R(0), R(0)};
      bool need = false;
      if (t < ntask && !L.npdone[slot]) {
        const int pj = L.nsij[slot];
        const int ti = pj & 255, tj = pj >> 8;
        const R tca[3] = {L.dc[DC_CX][ti], L.dc[DC_CY][ti], L.dc[DC_CZ][ti]};
        const R taa[3] = {L.dc[DC_AX][ti], L.dc[DC_AY][ti], L.dc[DC_AZ][ti]};
        const R tcb[3] = {L.dc[DC_CX][tj], L.dc[DC_CY][tj], L.dc[DC_CZ][tj]};
        const R tab[3] = {L.dc[DC_AX][tj], L.dc[DC_AY][tj], L.dc[DC_AZ][tj]};
        NpPair<R> q;
        np_pair(tca, taa, tcb, tab, q);
        bool far_a, far_b;
        np_far(q, r, h, far_a, far_b);
        need = rim < 2 || (rim == 2 ? far_a : far_b);
        if (need) np_rim_task(q, rim, k, r, h, f, x, y);
      }
      // the rim's result: the lowest start within RIM_SAME of the group's smallest f (bullet_mb.rim_closest)
      R fmin = f;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) fmin = g_min1(fmin, __shfl_xor(fmin, o));
      const unsigned long long near = __ballot(f <= fmin * (R(1) + NpTol<R>::same));
      const int g0 = ln & ~15;
      const int src = g0 + __builtin_ctz((unsigned)((near >> g0) & 0xffffull) | 0x10000u);
#pragma unroll
      for (int e = 0; e < 3; ++e) { x[e] = __shfl(x[e], src); y[e] = __shfl(y[e], src); }
      if (t < ntask && (t & 15) == 0) {
#pragma unroll
        for (int e = 0; e < 3; ++e) { L.DC_RIM(rim, e)[slot] = x[e]; L.DC_RIM(rim, 3 + e)[slot] = y[e]; }
        L.DC_RIM(rim, 6)[slot] = need ? R(0) : R(INFINITY);   // a rim the pair does not need
      }
    }
    wave_lds_sync();
#ifdef GPD_CONTACT_STATS
    const unsigned long long tn1 = __builtin_readcyclecounter();
    tn_task += tn1 - tn0;
#endif
    if (!found) {
      bool far_a, far_b;
      np_far(own, r, h, far_a, far_b);
      R cx[3][3], cy[3][3], cd[3];
      np_closed(own, r, h, far_a, far_b, cx, cy, cd);
      R ds[7];
      ds[0] = cd[0]; ds[1] = cd[1]; ds[2] = cd[2];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const R dx = L.DC_RIM(m, 0)[ln] - L.DC_RIM(m, 3)[ln], dy = L.DC_RIM(m, 1)[ln] - L.DC_RIM(m, 4)[ln],
                dz = L.DC_RIM(m, 2)[ln] - L.DC_RIM(m, 5)[ln];
        ds[3 + m] = L.DC_RIM(m, 6)[ln] == R(0) ? g_sqrt(pc_dot(dx, dy, dz, dx, dy, dz)) : R(INFINITY);
      }
      R dmin = ds[0];
#pragma unroll
      for (int m = 1; m < 7; ++m) dmin = g_min1(dmin, ds[m]);
      const R lim = dmin + NpTol<R>::tie;
      int w = 6;
#pragma unroll
      for (int m = 6; m >= 0; --m) w = ds[m] <= lim ? m : w;
      R bx[3], by[3], bd = ds[0];
#pragma unroll
      for (int e = 0; e < 3; ++e) { bx[e] = cx[0][e]; by[e] = cy[0][e]; }
#pragma unroll
      for (int m = 1; m < 7; ++m) {
        if (w == m) {
          bd = ds[m];
#pragma unroll
          for (int e = 0; e < 3; ++e) {
            bx[e] = m < 3 ? cx[m < 3 ? m : 0][e] : L.DC_RIM(m >= 3 ? m - 3 : 0, e)[ln];
            by[e] = m < 3 ? cy[m < 3 ? m : 0][e] : L.DC_RIM(m >= 3 ? m - 3 : 0, 3 + e)[ln];
          }
        }
      }
      yl[0] = by[0]; yl[1] = by[1]; yl[2] = by[2];
      if (bd > R(1e-4)) {
        found = true;
        mgf = mg;
        const R ux = (bx[0] - by[0]) / bd, uy = (bx[1] - by[1]) / bd, uz = (bx[2] - by[2]) / bd;
        n[0] = (ux * own.bp[0] + uy * own.bq[0]) + uz * ab[0];
        n[1] = (ux * own.bp[1] + uy * own.bq[1]) + uz * ab[1];
        n[2] = (ux * own.bp[2] + uy * own.bq[2]) + uz * ab[2];
        const R wx = (by[0] * own.bp[0] + by[1] * own.bq[0]) + by[2] * ab[0],
                wy = (by[0] * own.bp[1] + by[1] * own.bq[1]) + by[2] * ab[1],
                wz = (by[0] * own.bp[2] + by[1] * own.bq[2]) + by[2] * ab[2];
        pb[0] = cb[0] + (wx + n[0] * mg); pb[1] = cb[1] + (wy + n[1] * mg); pb[2] = cb[2] + (wz + n[2] * mg);
        dist = bd - R(2) * mg;
#ifdef GPD_CONTACT_STATS
        atomicAdd(&g_pc_hist[249 + lv], 1ull);   // narrowphases ending at margin level lv
#endif
      }
    }
    L.npdone[ln] = found ? 1 : 0;
    wave_lds_sync();
#ifdef GPD_CONTACT_STATS
    tn0 = __builtin_readcyclecounter();
    tn_sel += tn0 - tn1;
#endif
  }
#ifdef GPD_CONTACT_STATS
  const unsigned long long tn2 = __builtin_readcyclecounter();
#endif
  if (!found) {   // cores overlapping at every level: the least-overlap fallback at the last level's point
    pb[0] = cb[0] + ((yl[0] * own.bp[0] + yl[1] * own.bq[0]) + yl[2] * ab[0]);
    pb[1] = cb[1] + ((yl[0] * own.bp[1] + yl[1] * own.bq[1]) + yl[2] * ab[1]);
    pb[2] = cb[2] + ((yl[0] * own.bp[2] + yl[1] * own.bq[2]) + yl[2] * ab[2]);
    np_fallback(ca, aa, cb, ab, c.cyl_r, c.cyl_hh, n, dist);
#ifdef GPD_CONTACT_STATS
    atomicAdd(&g_pc_hist[253], 1ull);   // narrowphases ending in the least-overlap fallback
#endif
  }
#ifdef GPD_CONTACT_STATS
  if (__lane_id() == __ffsll((long long)__ballot(1)) - 1) {
    atomicAdd(&g_pc_hist[kPcNp + 0], 1ull);          // passes
    atomicAdd(&g_pc_hist[kPcNp + 1], tn_task);       // rim-task phases (all levels)
    atomicAdd(&g_pc_hist[kPcNp + 2], tn_sel);        // selections (all levels)
    atomicAdd(&g_pc_hist[kPcNp + 3], (unsigned long long)nthis);
    atomicAdd(&g_pc_hist[kPcNp + 4], __builtin_readcyclecounter() - tn2);   // fallback + face points (to here)
  }
#endif
  if (!mine) return 0;
  const R brk = c.brk;
  const bool con = dist < brk;
  R fp[4][3], fd[4];
  const bool face = con && mgf > R(0) && face_points(ca, aa, cb, ab, n, c.cyl_r, c.cyl_hh, mgf, fp, fd);
  int fmask = 0;
#pragma unroll
  for (int m = 0; m < 4; ++m) fmask |= (face && fd[m] < brk) ? (1 << m) : 0;
  // at most four points per pair, Bullet's MANIFOLD_CACHE_SIZE (bullet_mb.pair_manifold): with all
  // four face points the closest point takes the slot btPersistentManifold::sortCachedPoints frees
  const int rep = fmask == 15 ? manifold_replace(pb, dist, n, fp, fd) : -1;
  L.DC_ST(DS_N)[ln] = n[0]; L.DC_ST(DS_N + 1)[ln] = n[1]; L.DC_ST(DS_N + 2)[ln] = n[2];
  L.DC_ST(DS_PB)[ln] = pb[0]; L.DC_ST(DS_PB + 1)[ln] = pb[1]; L.DC_ST(DS_PB + 2)[ln] = pb[2];
  L.DC_ST(DS_D)[ln] = dist;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    L.DC_ST(DS_FP + 3 * m)[ln] = fp[m][0]; L.DC_ST(DS_FP + 3 * m + 1)[ln] = fp[m][1]; L.DC_ST(DS_FP + 3 * m + 2)[ln] = fp[m][2];
    L.DC_ST(DS_FD + m)[ln] = fd[m];
  }
  L.nsp[ln] = fmask | ((rep + 1) << 4);   // reused (the pair index is no longer needed): face-point
                                          // mask, and 1 + the slot the closest point replaces (0: none)
  return con ? (rep >= 0 ? 4 : 1 + __popc(fmask)) : 0;
}
template <typename R>
__device__ __noinline__ int dc_narrow_pass(const Consts<R>* cp, int ln, int nthis) {
  return dc_narrow_pass_body<R>(cp, ln, nthis);
}
// plane: the ground plane is on (the island solve takes the plane rows of drones in a pair contact
// that touch it, bullet_mb.drone_contact(plane=True)); nact: the block's drones
template <typename R, bool STAGE, bool INL>
__device__ __forceinline__ void dc_solve_body(const Consts<R>* cp, R inv_m, R dt, int ln, DcPairs dp, bool plane) {
#ifdef GPD_CONTACT_STATS
  const unsigned long long t0 = __builtin_readcyclecounter();
  unsigned long long t1 = t0, t2 = t0, t_np = t0;
  int n_near = 0;
#endif
  DcLds<R>& L = dc_lds<R>();
  const Consts<R>& c = *cp;
  const R idt = g_rcp(dt);
  const int nenv = dp.P > 0 ? dp.npairs / dp.P : 0;
  L.dc[DC_DLX][ln] = R(0); L.dc[DC_DLY][ln] = R(0); L.dc[DC_DLZ][ln] = R(0);
  L.dc[DC_DAX][ln] = R(0); L.dc[DC_DAY][ln] = R(0); L.dc[DC_DAZ][ln] = R(0);
  L.stouch[ln] = 0;
  L.island[ln] = 0;
  // ---- narrowphases: the near pairs compacted (pair order kept), near pair k to lane k % 64 of
  // pass k / 64; each contact pair emits its closest point and its face manifold's points below the
  // breaking threshold as consecutive contacts.  Contact c's rows are set up by lane c % 64: the
  // first 128 contacts in the lanes' registers (two rows a lane), later ones in the block's global
  // row store.
  int nnear = 0;
  for (int ch = 0; ch < dp.nch; ++ch) nnear += __popcll(L.nearw[ch]);
  if (ln < nenv) { L.ecnt[ln] = 0; L.ek0[ln] = 0x7fffffff; L.ek1[ln] = 0; }
  const int npass = (nnear + kWave - 1) / kWave;
  DcRow<R> w0, w1;
  bool have0 = false, have1 = false;
  w0.i = w0.j = w1.i = w1.j = 0;
  w0.rank = w1.rank = 0;
  R* rows = reinterpret_cast<R*>(dp.rows);
  constexpr int kRowR = dc_row_reals<R>();
  int ncon = 0;   // contacts emitted so far (wave-uniform)
  for (int ps = 0; ps < npass; ++ps) {
    int base = -ps * kWave;
    for (int ch = 0; ch < dp.nch; ++ch) {
      const unsigned long long nw = L.nearw[ch];
      if ((nw >> ln) & 1ull) {
        const int k = base + __popcll(nw & ((1ull << ln) - 1ull));
        if (k >= 0 && k < kWave) {
          const int p = ln + kWave * ch;
          L.nsp[k] = p;
          L.nsij[k] = dc_pair_of(dp, ch, p);
        }
      }
      base += __popcll(nw);
    }
    wave_lds_sync();
    const int nthis = nnear - ps * kWave < kWave ? nnear - ps * kWave : kWave;
#ifdef GPD_CONTACT_STATS
    n_near += ln < nthis ? 1 : 0;
#endif
    const int cnt = INL ? dc_narrow_pass_body<R>(cp, ln, nthis) : dc_narrow_pass<R>(cp, ln, nthis);
    int total;
    const int off = wave_excl_scan(cnt, ln, total);
    if (cnt > 0) {
      const int fmask = L.nsp[ln] & 15, rep = (L.nsp[ln] >> 4) - 1;
      int q = off;
      if (rep < 0) L.qmap[q++] = ln;          // the closest point first, then the face points
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if ((fmask >> m) & 1) L.qmap[q++] = m == rep ? ln : ln | ((m + 1) << 8);
    }
    wave_lds_sync();
#ifdef GPD_CONTACT_STATS
    if (ps == 0) t_np = __builtin_readcyclecounter();   // narrowphases of pass 0 done
#endif
    // the pass's contacts: contact c = ncon + q set up by lane c % 64
    for (int t = 0; t * kWave < total; ++t) {
      const int q = ((ln - ncon) & (kWave - 1)) + kWave * t;
      if (q < total) {
        const int cc = ncon + q;
        const int qm = L.qmap[q];
        const int sl = qm & 255, m = qm >> 8;
        const int pj = L.nsij[sl];
        const int i = pj & 255, j = pj >> 8;
        const R n[3] = {L.DC_ST(DS_N)[sl], L.DC_ST(DS_N + 1)[sl], L.DC_ST(DS_N + 2)[sl]};
        R pb[3], dist;
        if (m == 0) {
          pb[0] = L.DC_ST(DS_PB)[sl]; pb[1] = L.DC_ST(DS_PB + 1)[sl]; pb[2] = L.DC_ST(DS_PB + 2)[sl];
          dist = L.DC_ST(DS_D)[sl];
        } else {
          pb[0] = L.DC_ST(DS_FP + 3 * (m - 1))[sl]; pb[1] = L.DC_ST(DS_FP + 3 * (m - 1) + 1)[sl];
          pb[2] = L.DC_ST(DS_FP + 3 * (m - 1) + 2)[sl];
          dist = L.DC_ST(DS_FD + (m - 1))[sl];
        }
        DcRow<R> w;
        dc_row_setup<STAGE>(L, i, j, n, pb, dist, c, inv_m, idt, w, cc < kWave ? cc : -1);
        w.env = i / dp.D;
        w.rank = 0;   // the level pass below re-ranks when some env holds two contacts
        if (cc < kWave) {
          w0 = w;
          have0 = true;
          L.cij[ln] = pj;
        } else if (cc < kDcRegRows * kWave) {
          w1 = w;
          have1 = true;
          L.cij1[ln] = pj;
        } else {
          dc_row_store(rows + (long long)(cc / kWave - kDcRegRows) * kWave * kRowR, ln, w);
        }
        L.stouch[i] = 1;
        L.stouch[j] = 1;
        atomicAdd(&L.ecnt[w.env], 1);
        atomicMin(&L.ek0[w.env], cc);
        atomicMax(&L.ek1[w.env], cc + 1);
      }
    }
    ncon += total;
    wave_lds_sync();   // this pass's near slots and staging are rewritten by the next one
  }
  const int ncpass = (ncon + kWave - 1) / kWave;
  for (int x = ln; x < ncpass; x += kWave) {
    const int lo = x * kWave, n_in = ncon - lo;
    L.contw[x] = n_in >= kWave ? ~0ull : ((1ull << n_in) - 1ull);
  }
  // ---- the island: drones in a pair contact that touch the plane bring their plane rows
  bool isl = false;
  if (plane) {
    wave_lds_sync();
    // a drone in contact whose lowest plane candidate is above the breaking threshold has no plane
    // row (the plane solve's own gate, contact_low, with its margin): no island, rows not formed
    bool low = false;
    if (L.stouch[ln]) {
      const R r8 = L.dc[DC_AZ][ln], h67 = g_max1(g_abs(L.dc[DC_R6][ln]), g_abs(L.dc[DC_R7][ln]));
      const R zc = (-r8 < R(0) ? -c.cyl_hh : c.cyl_hh) + c.cyl_zoff;
      low = (L.dc[DC_PZ][ln] + r8 * zc) - c.cyl_r * h67 < c.brk + R(1e-6);
    }
    if (__ballot(low) != 0ull && low) isl = island_rows<STAGE>(L, ln, c, inv_m, idt);
    L.island[ln] = isl ? 1 : 0;
  }
  const bool any_isl = __ballot(isl) != 0ull;
  wave_lds_sync();
#ifdef GPD_CONTACT_STATS
  t1 = __builtin_readcyclecounter();
#endif
  // the largest contact count of an env
  int maxcnt = ln < nenv ? L.ecnt[ln] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int x = __shfl_xor(maxcnt, o);
    maxcnt = x > maxcnt ? x : maxcnt;
  }
  // Gauss-Seidel levels (only when some env holds two contacts): a contact's level is one more
  // than the highest level among the earlier contacts (in (i, j) order) that share a drone with it.
  // Contacts of one level share no drone, so solving a level's contacts at once and the levels in
  // order IS the sequential sweep over the env's contacts (non-adjacent rows of disjoint drones
  // commute) - a pile of contacts through one drone still takes one round per contact, independent
  // pairs of one env take one; a pair's points (same two drones) take one round each.
  int rounds = maxcnt;
  if (maxcnt > 1) {
    L.dlev[ln] = 0;
    L.clev[ln] = 0;
    L.clev1[ln] = 0;
    wave_lds_sync();
    int lmax = ln < nenv && L.ecnt[ln] > 0 ? 1 : 0;
    if (ln < nenv && L.ecnt[ln] > 1) {
      for (int k = L.ek0[ln]; k < L.ek1[ln]; ++k) {
        int pij;
        int* ints = nullptr;
        if (k < kWave) {
          pij = L.cij[k];
        } else if (k < kDcRegRows * kWave) {
          pij = L.cij1[k - kWave];
        } else {
          ints = reinterpret_cast<int*>(rows + (long long)(k / kWave - kDcRegRows) * kWave * kRowR + kRowReal * kWave) +
                 (k & (kWave - 1));
          pij = ints[0] | (ints[kWave] << 8);
        }
        const int i = pij & 255, j = pij >> 8;
        const int li = L.dlev[i], lj = L.dlev[j];
        const int lev = (li > lj ? li : lj) + 1;
        L.dlev[i] = lev;
        L.dlev[j] = lev;
        if (k < kWave) L.clev[k] = lev - 1;
        else if (k < kDcRegRows * kWave) L.clev1[k - kWave] = lev - 1;
        else ints[3 * kWave] = lev - 1;
        lmax = lev > lmax ? lev : lmax;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int x = __shfl_xor(lmax, o);
      lmax = x > lmax ? x : lmax;
    }
    rounds = lmax;
    wave_lds_sync();
    if (have0) w0.rank = L.clev[ln];
    if (have1) w1.rank = L.clev1[ln];
  }
  const R mu = c.dd_mu, resid = c.resid, pmu = c.mu;
  const int iters = c.iters;
#ifdef GPD_CONTACT_STATS
  t2 = __builtin_readcyclecounter();
  int it_used = 0;
#endif
  if (maxcnt <= 1 && ncpass <= 1 && !any_isl) {
    // ---- every env has at most one contact and no island: its lane owns both drones' deltas
    R vi[6] = {R(0), R(0), R(0), R(0), R(0), R(0)}, vj[6] = {R(0), R(0), R(0), R(0), R(0), R(0)};
    DcInv<R> I0;
    if (!STAGE) dc_inv(L, w0.i, w0.j, I0);
    bool done = !have0;
    for (int it = 0; it < iters; ++it) {
      if (__ballot(!done) == 0ull) break;
#ifdef GPD_CONTACT_STATS
      it_used = it + 1;
#endif
      if (!done) {
        R res;
        if (STAGE) {
          const DcJacLds<R> J0{dc_stage<R>(), ln};
          res = dc_normal(w0, inv_m, vi, vj, J0);
          res = g_fmax(res, dc_friction(w0, mu, inv_m, vi, vj, J0));
        } else {
          const DcJacRow<R> J0{w0, I0};
          res = dc_normal(w0, inv_m, vi, vj, J0);
          res = g_fmax(res, dc_friction(w0, mu, inv_m, vi, vj, J0));
        }
        done = res <= resid;
      }
    }
    if (have0) {
      L.dc[DC_DLX][w0.i] = vi[0]; L.dc[DC_DLY][w0.i] = vi[1]; L.dc[DC_DLZ][w0.i] = vi[2];
      L.dc[DC_DAX][w0.i] = vi[3]; L.dc[DC_DAY][w0.i] = vi[4]; L.dc[DC_DAZ][w0.i] = vi[5];
      L.dc[DC_DLX][w0.j] = vj[0]; L.dc[DC_DLY][w0.j] = vj[1]; L.dc[DC_DLZ][w0.j] = vj[2];
      L.dc[DC_DAX][w0.j] = vj[3]; L.dc[DC_DAY][w0.j] = vj[4]; L.dc[DC_DAZ][w0.j] = vj[5];
    }
  } else {
    // ---- general case: per phase (normal rows, then friction pairs) the island drones' plane rows
    // (one round: each drone's own rows), then round r solves the level-r contacts of every env;
    // deltas through LDS (bullet_mb.drone_contact's order: plane normal, pair normal, plane
    // friction, pair friction)
    if (ln < nenv) { L.edone[ln] = L.ecnt[ln] == 0; L.eres[ln] = R(0); }
    wave_lds_sync();
    R vi[6], vj[6];
    // one row: deltas from LDS, the row's step, deltas back; its squared residual
    auto visit = [&](DcRow<R>& w, bool friction, int slot) -> R {
#pragma unroll
      for (int x = 0; x < 6; ++x) { vi[x] = L.dc[DC_DLX + x][w.i]; vj[x] = L.dc[DC_DLX + x][w.j]; }
      R rr;
      if (STAGE && slot >= 0) {
        const DcJacLds<R> J{dc_stage<R>(), slot};
        rr = friction ? dc_friction(w, mu, inv_m, vi, vj, J) : dc_normal(w, inv_m, vi, vj, J);
      } else {
        DcInv<R> I;
        dc_inv(L, w.i, w.j, I);
        const DcJacRow<R> J{w, I};
        rr = friction ? dc_friction(w, mu, inv_m, vi, vj, J) : dc_normal(w, inv_m, vi, vj, J);
      }
#pragma unroll
      for (int x = 0; x < 6; ++x) { L.dc[DC_DLX + x][w.i] = vi[x]; L.dc[DC_DLX + x][w.j] = vj[x]; }
      return rr;
    };
    const int my_env = ln / dp.D;
#ifdef GPD_CONTACT_STATS
    unsigned long long tg_isl = 0, tg_nrm = 0, tg_fr = 0, tg_end = 0, tg0 = __builtin_readcyclecounter();
#endif
    for (int it = 0; it < iters; ++it) {
      // edone / eres of every env are settled here (the previous iteration's end)
      if (__ballot(ln < nenv && !L.edone[ln]) == 0ull) break;
#ifdef GPD_CONTACT_STATS
      it_used = it + 1;
#endif
      // the envs still iterating, read once per iteration; each lane's residuals per env in registers
      const bool live0 = have0 && !L.edone[w0.env], live1 = have1 && !L.edone[w1.env];
      const bool livei = isl && !L.edone[my_env];
      R res0 = R(0), res1 = R(0), resi = R(0);
      for (int ph = 0; ph < 2; ++ph) {              // normal rows, then friction pairs
#ifdef GPD_CONTACT_STATS
        const unsigned long long tga = __builtin_readcyclecounter();
        tg_end += tga - tg0;
#endif
        if (any_isl) {
          if (livei) resi = g_fmax(resi, island_sweep<STAGE>(L, ln, ph == 1, pmu, inv_m));
          wave_lds_sync();
        }
#ifdef GPD_CONTACT_STATS
        const unsigned long long tgb = __builtin_readcyclecounter();
        tg_isl += tgb - tga;
#endif
        for (int r = 0; r < rounds; ++r) {
          if (live0 && w0.rank == r) res0 = g_fmax(res0, visit(w0, ph == 1, ln));
          if (live1 && w1.rank == r) res1 = g_fmax(res1, visit(w1, ph == 1, -1));
          for (int ch = kDcRegRows; ch < ncpass; ++ch) {
            if (((L.contw[ch] >> ln) & 1ull) == 0) continue;
            R* chunk = rows + (long long)(ch - kDcRegRows) * kWave * kRowR;
            if (reinterpret_cast<const int*>(chunk + kRowReal * kWave)[3 * kWave + ln] != r) continue;   // its rank
            DcRow<R> w;
            dc_row_load(chunk, ln, w);
            if (L.edone[w.env]) continue;
            eres_max(L, w.env, visit(w, ph == 1, -1));
#pragma unroll
            for (int q = 0; q < 3; ++q) chunk[(kRowLam + q) * kWave + ln] = w.lam[q];
          }
          wave_lds_sync();
        }
#ifdef GPD_CONTACT_STATS
        tg0 = __builtin_readcyclecounter();
        if (ph == 0) tg_nrm += tg0 - tgb; else tg_fr += tg0 - tgb;
#endif
      }
      if (live0) eres_max(L, w0.env, res0);
      if (live1) eres_max(L, w1.env, res1);
      if (livei) eres_max(L, my_env, resi);
      wave_lds_sync();
      if (ln < nenv) {
        if (!L.edone[ln]) L.edone[ln] = L.eres[ln] <= resid;
        L.eres[ln] = R(0);
      }
      wave_lds_sync();
    }
#ifdef GPD_CONTACT_STATS
    tg_end += __builtin_readcyclecounter() - tg0;
    if (__lane_id() == __ffsll((long long)__ballot(1)) - 1) {
      atomicAdd(&g_pc_hist[kPcNp + 7], tg_isl);    // general path: island sweeps
      atomicAdd(&g_pc_hist[kPcNp + 8], tg_nrm);    // normal rounds
      atomicAdd(&g_pc_hist[kPcNp + 9], tg_fr);     // friction rounds
      atomicAdd(&g_pc_hist[kPcNp + 10], tg_end);   // iteration ends (convergence checks)
      atomicAdd(&g_pc_hist[kPcNp + 11], (unsigned long long)it_used * rounds);   // rounds per phase run
      atomicAdd(&g_pc_hist[kPcNp + 12], (unsigned long long)it_used);            // general-path iterations
    }
#endif
  }
#ifdef GPD_CONTACT_STATS
  {
    const unsigned long long t3 = __builtin_readcyclecounter();
    int tot = n_near;
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    if (__lane_id() == __ffsll((long long)__ballot(1)) - 1) {
      atomicAdd(&g_pc_hist[116], 1ull);
      atomicAdd(&g_pc_hist[117], t2 - t0);
      atomicAdd(&g_pc_hist[118], t3 - t2);
      atomicAdd(&g_pc_hist[119], (unsigned long long)it_used);
      atomicAdd(&g_pc_hist[123], t1 - t0);
      atomicAdd(&g_pc_hist[254], t_np - t0);   // to the end of pass 0's narrowphases
      atomicAdd(&g_pc_hist[126], (unsigned long long)ncon);
      atomicAdd(&g_pc_hist[127], (unsigned long long)tot);
      atomicAdd(&g_pc_hist[124], any_isl ? 1ull : 0ull);                                   // island solves
      atomicAdd(&g_pc_hist[125], (maxcnt <= 1 && ncpass <= 1 && !any_isl) ? 1ull : 0ull);  // register fast path
      atomicAdd(&g_pc_hist[243], (unsigned long long)rounds);                               // GS rounds per phase
      atomicMax(&g_pc_hist[255], (unsigned long long)ncon);                                 // most contacts of a solve
      atomicAdd(&g_pc_hist[kPcNp + 5], ncon > kDcRegRows * kWave ? 1ull : 0ull);           // solves using the row store
      atomicAdd(&g_pc_hist[kPcNp + 6], (unsigned long long)ncpass);
      const unsigned long long cyc = t3 - t0;
      atomicAdd(&g_pc_hist[128 + (63 - __clzll(cyc | 1ull))], 1ull);
      atomicAdd(&g_pc_hist[192 + it_used], 1ull);
      if (blockIdx.x < 4096) atomicAdd(&g_pc_hist[256 + blockIdx.x], cyc);
    }
  }
#endif
  wave_lds_sync();   // the caller reads the velocity deltas
}
// the solve as a call (its registers out of the caller's allocation; the run-time-flag kernels and
// the downwash flag sets)
template <typename R, bool STAGE>
__device__ __noinline__ void dc_solve(const Consts<R>* cp, R inv_m, R dt, int ln, DcPairs dp, bool plane) {
  dc_solve_body<R, STAGE, false>(cp, inv_m, dt, ln, dp, plane);
}
// the hook bullet_substep calls (multi-drone envs of one-wave blocks): pk parks the caller's
// values in LDS around the solve (bullet_substep), so nothing of the substep loop is live across
// the call and the loop's own register allocation does not see the solve.  INL: the solve and its
// narrowphase inlined (no call, no callee-saved register spills): the compiled-in PYB flag sets
// without downwash - the 2-drone MultiHover PYB batch 127.1 -> 119.5 us, while the 8-drone
// PYB_GND_DRAG_DW batch, whose island sweeps then share the kernel's register allocation, went
// 3 103 -> 3 535 us (profiles/r6/contact/probe_inline_ab.log); inlined only here: 2-drone
// 126.7 -> 119.9 us, 8-drone PYB 16.3 -> 14.2 us, 8-drone PYB_GND_DRAG_DW unchanged (probe_selective_inline_ab.log)
template <bool INL>
struct DcHookT {
  int tid;
  DcPairs dp;
  // returns whether this lane's drone joined the island (its plane rows were solved here)
  template <typename R, class PK>
  __device__ __forceinline__ bool operator()(Drone<R>& s, R* Rm, const Consts<R>& c, const DynK<R>& k, const PK& pk,
                                             bool plane) const {
    DcLds<R>& L = dc_lds<R>();
    const DcPairs& P = dp;
    const int ln = tid & (kWave - 1);
    const R zo = c.cyl_zoff;
    L.dc[DC_CX][ln] = s.px + Rm[2] * zo; L.dc[DC_CY][ln] = s.py + Rm[5] * zo; L.dc[DC_CZ][ln] = s.pz + Rm[8] * zo;
    L.dc[DC_AX][ln] = Rm[2]; L.dc[DC_AY][ln] = Rm[5]; L.dc[DC_AZ][ln] = Rm[8];
    wave_lds_sync();
    bool any = false, isl = false;
    for (int ch = 0; ch < P.nch; ++ch) {
      const int p = ln + kWave * ch;
      bool near = false;
      if (p < P.npairs) {
        const int pij = dc_pair_of(P, ch, p);
        near = dc_near(L, pij & 255, pij >> 8, c);
      }
      const unsigned long long w = __ballot(near);
      if (ln == 0) L.nearw[ch] = w;
      any = any || w != 0ull;
    }
    if (GPD_RARE(any)) {
#ifdef GPD_CONTACT_STATS
      const unsigned long long tr0 = __builtin_readcyclecounter();
#endif
      // this lane's columns for the solve: pose, velocities, world inverse inertia R diag(1/I) R^T
      const R q00 = k.ijx * Rm[0], q01 = k.ijy * Rm[1], q02 = k.ijz * Rm[2];
      const R q10 = k.ijx * Rm[3], q11 = k.ijy * Rm[4], q12 = k.ijz * Rm[5];
      const R q20 = k.ijx * Rm[6], q21 = k.ijy * Rm[7], q22 = k.ijz * Rm[8];
      L.dc[DC_I00][ln] = pc_dot(q00, q01, q02, Rm[0], Rm[1], Rm[2]);
      L.dc[DC_I01][ln] = pc_dot(q00, q01, q02, Rm[3], Rm[4], Rm[5]);
      L.dc[DC_I02][ln] = pc_dot(q00, q01, q02, Rm[6], Rm[7], Rm[8]);
      L.dc[DC_I11][ln] = pc_dot(q10, q11, q12, Rm[3], Rm[4], Rm[5]);
      L.dc[DC_I12][ln] = pc_dot(q10, q11, q12, Rm[6], Rm[7], Rm[8]);
      L.dc[DC_I22][ln] = pc_dot(q20, q21, q22, Rm[6], Rm[7], Rm[8]);
      L.dc[DC_PX][ln] = s.px; L.dc[DC_PY][ln] = s.py; L.dc[DC_PZ][ln] = s.pz;
      L.dc[DC_VX][ln] = s.vx; L.dc[DC_VY][ln] = s.vy; L.dc[DC_VZ][ln] = s.vz;
      L.dc[DC_WX][ln] = s.wx; L.dc[DC_WY][ln] = s.wy; L.dc[DC_WZ][ln] = s.wz;
      L.dc[DC_R0][ln] = Rm[0]; L.dc[DC_R1][ln] = Rm[1]; L.dc[DC_R3][ln] = Rm[3];
      L.dc[DC_R4][ln] = Rm[4]; L.dc[DC_R6][ln] = Rm[6]; L.dc[DC_R7][ln] = Rm[7];
      const R inv_m = k.inv_m, dt = k.dt;
      const DcPairs dpc = P;
      wave_lds_sync();
#ifdef GPD_CONTACT_STATS
      const unsigned long long tr1 = __builtin_readcyclecounter();
#endif
      pk.park();
#ifdef GPD_CONTACT_STATS
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const unsigned long long tr2 = __builtin_readcyclecounter();
#endif
      if (INL) dc_solve_body<R, PK::kStage, true>(&c, inv_m, dt, ln, dpc, plane);
      else dc_solve<R, PK::kStage>(&c, inv_m, dt, ln, dpc, plane);
#ifdef GPD_CONTACT_STATS
      const unsigned long long tr3 = __builtin_readcyclecounter();
#endif
      pk.unpark();
      isl = L.island[ln] != 0;
      if (L.stouch[ln]) {
        s.vx = s.vx + L.dc[DC_DLX][ln]; s.vy = s.vy + L.dc[DC_DLY][ln]; s.vz = s.vz + L.dc[DC_DLZ][ln];
        s.wx = s.wx + L.dc[DC_DAX][ln]; s.wy = s.wy + L.dc[DC_DAY][ln]; s.wz = s.wz + L.dc[DC_DAZ][ln];
      }
#ifdef GPD_CONTACT_STATS
      {
        const unsigned long long tr4 = __builtin_readcyclecounter();
        if (ln == 0) {
          if (blockIdx.x < 4096) atomicAdd(&g_pc_hist[256 + 12288 + blockIdx.x], tr4 - tr0);
          atomicAdd(&g_pc_hist[244], tr1 - tr0);   // columns for the solve
          atomicAdd(&g_pc_hist[245], tr2 - tr1);   // park
          atomicAdd(&g_pc_hist[246], tr3 - tr2);   // the call (the solve included)
          atomicAdd(&g_pc_hist[247], tr4 - tr3);   // unpark + deltas
          atomicAdd(&g_pc_hist[248], 1ull);
        }
      }
#endif
    }
    wave_lds_sync();   // the centre columns are rewritten by the next substep
    return isl;
  }
};

}  // namespace gpd
