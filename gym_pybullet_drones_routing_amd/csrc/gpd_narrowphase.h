// gpd_narrowphase.h — the cylinder x cylinder narrowphase of the drone <-> drone contact
// (cyl_extent_cos ... manifold_replace): closest points of two drones' collision cylinders, the
// cap-to-cap face manifold and its replacement rule.  Pure per-pair functions in registers; needs
// only the math of gpd_device.h.  The comment below introduces the whole contact restatement,
// whose broadphase, rows and solve are in gpd_dcontact.h.
#pragma once
#include "gpd_layout.h"

namespace gpd {

// ---------------------------------------------------------------- drone <-> drone contact (PYB*, D > 1)
// MultiHoverAviary's drones are colliding Bullet bodies (BaseAviary.py:486-491) stepped together
// by p.stepSimulation() (:369-370).  Restatement (oracle/bullet_mb.py drone_contact; parity
// unpinned like the plane's: Bullet's GJK / EPA and its persistent manifold are not restated):
//   * broadphase (pair_near): pairs (i, j > i) of an env whose bounding spheres come within the
//     breaking threshold and that no separating axis (the two cylinder axes, the centre line)
//     keeps farther apart than it;
//   * narrowphase: Bullet's margin scheme, the CONVERGED closest points of the margin-shrunk core
//     cylinders (core_pair: cap centres, lateral surfaces, the four rims by trust-region Newton)
//     give the normal (B -> A) and distance core - 2 x margin, with thicker margins for deeper
//     overlaps (up to ~2 cm), beyond that the least overlap over the centre line and the two axes;
//   * a cap-to-cap contact adds its face manifold (face_points: four points spanning the caps'
//     overlap), each point below the breaking threshold a contact of the pair; at most four points
//     per pair (Bullet's MANIFOLD_CACHE_SIZE): with four face points the closest point replaces the
//     one sortCachedPoints would (manifold_replace);
//   * EVERY pair whose distance is below the breaking threshold is in contact (up to kDcPts
//     contacts per pair), solved in (i, j) order;
//   * rows (normal, btPlaneSpace1 friction pair) between two bodies: effective mass
//     2/m + a_A.I_A^-1 a_A + a_B.I_B^-1 a_B; the plane's rhs rules and cone (mu 0.25); projected
//     Gauss-Seidel over the env's normal rows, then friction pairs, in contact order; the env stops
//     at its largest squared residual <= resid or after `iters` iterations;
//   * island: a drone in a pair contact that touches the ground plane brings its plane rows into
//     the env's loop (plane normal rows, pair normal rows, plane friction, pair friction per
//     iteration, as Bullet solves an island), and skips its own plane solve.
// GPU layout.  The pairs of a block's whole envs are numbered p = env * P + q (P = D(D-1)/2, q the
// (i, j) index of bullet_mb.drone_contacts' order) and lane ln handles pairs ln, ln + 64, ... (chunk
// ch = p / 64).  The hot part (DcHook, every substep): the drones' centre / axis columns into LDS,
// the broadphase of every pair (the sphere test; the separating-axis tests only for pairs in
// reach), one ballot per chunk.  A wave with a pair in reach calls dc_solve (rare): its near pairs
// compacted over the lanes (in pair order, whatever chunk they come from), the narrowphase of up to
// 64 of them per pass in parallel, their contacts (closest point + face points) numbered in order
// and each set up by lane c % 64 - the first 64 in registers, later ones in a per-block global row
// store - then the Gauss-Seidel sweeps: round r solves the level-r contacts of every env at once
// (contacts of one level touch different drones), the drones' velocity deltas in LDS.  When no env
// of the wave has more than one contact (no face manifold, no island) the owner lane keeps its two
// drones' deltas in registers for the whole solve and the sweep needs no LDS at all.
template <typename R>
__device__ __forceinline__ R cyl_extent_cos(R ua, R r, R hh) {
  const R s2 = R(1) - ua * ua;
  return hh * g_abs(ua) + r * g_sqrt(s2 > R(0) ? s2 : R(0));
}
// btPlaneSpace1
template <typename R>
__device__ __forceinline__ void plane_space(const R n[3], R p[3], R q[3]) {
  if (g_abs(n[2]) > R(0.7071067811865475244008443621048490)) {
    const R a = n[1] * n[1] + n[2] * n[2];
    const R k = g_rsqrt(a);   // ~2 ulp from 1 / sqrt(a), a third of the instructions
    p[0] = R(0); p[1] = -n[2] * k; p[2] = n[1] * k;
    q[0] = a * k; q[1] = -n[0] * p[2]; q[2] = n[0] * p[1];
  } else {
    const R a = n[0] * n[0] + n[1] * n[1];
    const R k = g_rsqrt(a);
    p[0] = -n[1] * k; p[1] = n[0] * k; p[2] = R(0);
    q[0] = -n[2] * p[1]; q[1] = n[2] * p[0]; q[2] = a * k;
  }
}

// ---- narrowphase (oracle/bullet_mb.py core_pair / rim_newton / rim_closest / pair_geometry / face_points)
// The closest points of the margin-shrunk cores, converged: the near caps' centres, the lateral
// surfaces along the axes' closest points (closed forms), and the four rim circles against the other
// cylinder - 5 trust-region Newton steps on the rim angle from each of 16 start azimuths (k x 22.5
// deg), the smallest squared distance per rim; the first candidate within the tie of the closest
// wins.  Everything in B's frame (btPlaneSpace1(aB), aB); B's rims in A's frame (btPlaneSpace1 of A).
// A pass's near pairs split into 64 tasks each (4 rims x 16 starts) over the wave's lanes
// (dc_narrow_pass): a sparse wave (one near pair, the common case) runs ONE Newton chain of 6
// evaluations per lane (round 5: 4 starts x 8 steps, 9 evaluations).
template <typename R> struct NpTol;
template <> struct NpTol<double> { static constexpr double accept = 1e-10, same = 1e-4, tie = 1e-7; };   // RIM_ACCEPT, RIM_SAME, PAIR_TIE
template <> struct NpTol<float> { static constexpr float accept = 1e-5f, same = 1e-4f, tie = 1e-7f; };
constexpr int kRimSamples = 16, kRimIters = 5;   // RIM_SAMPLES, RIM_ITERS
template <typename R>
__device__ __forceinline__ void axial_project(R x, R y, R z, R r, R h, R& qx, R& qy, R& qz) {
  const R rho2 = x * x + y * y;
  const R f = rho2 > r * r ? r / g_sqrt(rho2) : R(1);
  qx = x * f; qy = y * f; qz = g_max1(g_min1(z, h), -h);
}
template <typename R>
__device__ __forceinline__ R axial_extent(R az, R r, R h) {
  const R s2 = R(1) - az * az;
  return h * g_abs(az) + r * g_sqrt(s2 > R(0) ? s2 : R(0));
}
// the rim point C + r (c e1 + s e2) against the axial cylinder: squared distance f, f'/2 = g and
// f''/2 = hh in the rim angle (bullet_mb._rim_eval), the point P and its projection Q
template <typename R>
struct RimEval {
  R f, g, hh, P[3], Q[3];
};
template <typename R>
__device__ __forceinline__ void rim_eval(const R C[3], const R e1[3], const R e2[3], R c, R s, R r, R h, RimEval<R>& o) {
  const R u0 = c * e1[0] + s * e2[0], u1 = c * e1[1] + s * e2[1], u2 = c * e1[2] + s * e2[2];
  const R d0 = r * (c * e2[0] - s * e1[0]), d1 = r * (c * e2[1] - s * e1[1]), d2 = r * (c * e2[2] - s * e1[2]);
  o.P[0] = C[0] + r * u0; o.P[1] = C[1] + r * u1; o.P[2] = C[2] + r * u2;
  const R rho2 = o.P[0] * o.P[0] + o.P[1] * o.P[1];
  const bool out_r = rho2 > r * r;
  const R ir = g_rsqrt(out_r ? rho2 : R(1));
  const R k = out_r ? r * ir : R(1);
  o.Q[0] = o.P[0] * k; o.Q[1] = o.P[1] * k; o.Q[2] = g_max1(g_min1(o.P[2], h), -h);
  const R e0 = o.P[0] - o.Q[0], e1_ = o.P[1] - o.Q[1], e2_ = o.P[2] - o.Q[2];
  o.f = pc_dot(e0, e1_, e2_, e0, e1_, e2_);
  o.g = pc_dot(e0, e1_, e2_, d0, d1, d2);
  const R rt = (o.P[0] * d0 + o.P[1] * d1) * (ir * ir);
  const R m0 = out_r ? d0 - k * (d0 - rt * o.P[0]) : R(0);
  const R m1 = out_r ? d1 - k * (d1 - rt * o.P[1]) : R(0);
  const R m2 = g_abs(o.P[2]) > h ? d2 : R(0);
  o.hh = pc_dot(m0, m1, m2, d0, d1, d2) - r * pc_dot(e0, e1_, e2_, u0, u1, u2);
}
// bullet_mb.rim_newton: kRimIters trust-region Newton steps on the rim angle from (c, s)
template <typename R>
__device__ __forceinline__ void rim_newton(const R C[3], const R e1[3], const R e2[3], R r, R h, R c, R s, RimEval<R>& cur) {
  constexpr R kAcc = NpTol<R>::accept;
  rim_eval(C, e1, e2, c, s, r, h, cur);
  R rad = R(0.19634954084936207);   // pi / RIM_SAMPLES
#pragma unroll 1
  for (int it = 0; it < kRimIters; ++it) {
    // -g / hh and 1 / sqrt as Newton-refined reciprocals (~1 ulp; the oracle divides)
    R d = cur.hh > R(0) ? -cur.g * g_rcp(cur.hh > R(0) ? cur.hh : R(1)) : -copysign(rad, cur.g);
    d = g_max1(g_min1(d, rad), -rad);
    R c2 = c - d * s, s2 = s + d * c;
    const R kn = g_rsqrt(c2 * c2 + s2 * s2);
    c2 = c2 * kn; s2 = s2 * kn;
    RimEval<R> nx;
    rim_eval(C, e1, e2, c2, s2, r, h, nx);
    const bool acc = nx.f < cur.f * (R(1) - kAcc);
    if (acc) { c = c2; s = s2; cur = nx; }
    rad = acc ? g_min1(R(2) * rad, R(1)) : g_abs(d) * R(0.25);
  }
}
// closest point of the cylinder (centre c, unit axis a) to x (bullet_mb.cyl_project)
template <typename R>
__device__ __forceinline__ void cyl_project(const R c[3], const R a[3], R r, R h, const R x[3], R o[3]) {
  const R dx = x[0] - c[0], dy = x[1] - c[1], dz = x[2] - c[2];
  const R t = pc_dot(dx, dy, dz, a[0], a[1], a[2]);
  const R tc = g_max1(g_min1(t, h), -h);
  R rx = dx - t * a[0], ry = dy - t * a[1], rz = dz - t * a[2];
  const R rho2 = pc_dot(rx, ry, rz, rx, ry, rz);
  const R f = rho2 > r * r ? r / g_sqrt(rho2) : R(1);
  o[0] = (c[0] + tc * a[0]) + rx * f; o[1] = (c[1] + tc * a[1]) + ry * f; o[2] = (c[2] + tc * a[2]) + rz * f;
}
// a pair in B's frame: A's centre L and axis A, B's world basis (bp, bq, ab); A's frame (ap, aq, A)
// with B's centre Lb and axis Bz in it and B's rim basis (bp2, bq2) there; the facing caps and
// which far rims (and the lateral pair) are needed (bullet_mb.core_pair)
template <typename R>
struct NpPair {
  R L[3], A[3], bp[3], bq[3], ap[3], aq[3], Lb[3], Bz[3], bp2[3], bq2[3];
  R la, sa, sb;
};
template <typename R>
__device__ __forceinline__ void np_pair(const R ca[3], const R aa[3], const R cb[3], const R ab[3], NpPair<R>& q) {
  plane_space(ab, q.bp, q.bq);
  const R lx = ca[0] - cb[0], ly = ca[1] - cb[1], lz = ca[2] - cb[2];
  q.L[0] = pc_dot(q.bp[0], q.bp[1], q.bp[2], lx, ly, lz); q.L[1] = pc_dot(q.bq[0], q.bq[1], q.bq[2], lx, ly, lz);
  q.L[2] = pc_dot(ab[0], ab[1], ab[2], lx, ly, lz);
  q.A[0] = pc_dot(q.bp[0], q.bp[1], q.bp[2], aa[0], aa[1], aa[2]); q.A[1] = pc_dot(q.bq[0], q.bq[1], q.bq[2], aa[0], aa[1], aa[2]);
  q.A[2] = pc_dot(ab[0], ab[1], ab[2], aa[0], aa[1], aa[2]);
  plane_space(q.A, q.ap, q.aq);
  q.Lb[0] = -pc_dot(q.ap[0], q.ap[1], q.ap[2], q.L[0], q.L[1], q.L[2]);
  q.Lb[1] = -pc_dot(q.aq[0], q.aq[1], q.aq[2], q.L[0], q.L[1], q.L[2]);
  q.Lb[2] = -pc_dot(q.A[0], q.A[1], q.A[2], q.L[0], q.L[1], q.L[2]);
  q.Bz[0] = q.ap[2]; q.Bz[1] = q.aq[2]; q.Bz[2] = q.A[2];
  plane_space(q.Bz, q.bp2, q.bq2);
  q.la = -q.Lb[2];
  q.sa = q.la > R(0) ? R(-1) : R(1);
  q.sb = q.L[2] >= R(0) ? R(1) : R(-1);
}
template <typename R>
__device__ __forceinline__ void np_far(const NpPair<R>& q, R r, R h, bool& far_a, bool& far_b) {
  far_a = -q.sa * q.la - h < axial_extent(q.sa * q.A[2], r, h);
  far_b = q.sb * q.L[2] - h < axial_extent(q.A[2], r, h);
}
template <typename R>
__device__ __forceinline__ void np_to_b(const NpPair<R>& q, const R v[3], R o[3]) {   // A's frame -> B's: Ma^T v + L
  o[0] = ((q.ap[0] * v[0] + q.aq[0] * v[1]) + q.A[0] * v[2]) + q.L[0];
  o[1] = ((q.ap[1] * v[0] + q.aq[1] * v[1]) + q.A[1] * v[2]) + q.L[1];
  o[2] = ((q.ap[2] * v[0] + q.aq[2] * v[1]) + q.A[2] * v[2]) + q.L[2];
}
// one rim task: rim 0/2 = A's near / far rim against B, 1/3 = B's near / far rim against A, from
// start azimuth k (k x 22.5 deg); (x on A, y on B) in B's frame and the squared distance
template <typename R>
__device__ __forceinline__ void np_rim_task(const NpPair<R>& q, int rim, int k, R r, R h, R& f, R x[3], R y[3]) {
  // bullet_mb.RIM_COS / RIM_SIN: the first quadrant's (cos, sin) turned by k / 4 quarter turns,
  // negations as 0 - x (+0.0 where the oracle's table has it)
  const R H = R(0.7071067811865475244008443621048490), C1 = R(0.92387953251128674), S1 = R(0.38268343236508978);
  const int qd = k & 3, qt = k >> 2;
  const R qc = qd == 0 ? R(1) : (qd == 1 ? C1 : (qd == 2 ? H : S1));
  const R qs = qd == 0 ? R(0) : (qd == 1 ? S1 : (qd == 2 ? H : C1));
  const R c0 = qt == 0 ? qc : (qt == 1 ? R(0) - qs : (qt == 2 ? R(0) - qc : qs));
  const R s0 = qt == 0 ? qs : (qt == 1 ? qc : (qt == 2 ? R(0) - qs : R(0) - qc));
  const bool on_a = (rim & 1) == 0;
  const R sg = on_a ? (rim < 2 ? q.sa : -q.sa) : (rim < 2 ? q.sb : -q.sb);
  const R* base = on_a ? q.L : q.Lb;
  const R* ax = on_a ? q.A : q.Bz;
  const R* e1 = on_a ? q.ap : q.bp2;
  const R* e2 = on_a ? q.aq : q.bq2;
  const R C[3] = {base[0] + sg * h * ax[0], base[1] + sg * h * ax[1], base[2] + sg * h * ax[2]};
  RimEval<R> o;
  rim_newton(C, e1, e2, r, h, c0, s0, o);
  f = o.f;
  if (on_a) {
    x[0] = o.P[0]; x[1] = o.P[1]; x[2] = o.P[2];
    y[0] = o.Q[0]; y[1] = o.Q[1]; y[2] = o.Q[2];
  } else {   // B's rim point P and A's point Q, both in A's frame
    np_to_b(q, o.Q, x);
    np_to_b(q, o.P, y);
  }
}
// the closed-form candidates 0..2 of bullet_mb.core_pair: the near caps' centres and the lateral pair
// (d = +inf where the lateral pair is not a candidate)
template <typename R>
__device__ __forceinline__ void np_closed(const NpPair<R>& q, R r, R h, bool far_a, bool far_b, R x[3][3], R y[3][3],
                                          R d[3]) {
  const R inf = R(INFINITY);
  x[0][0] = q.L[0] + q.sa * h * q.A[0]; x[0][1] = q.L[1] + q.sa * h * q.A[1]; x[0][2] = q.L[2] + q.sa * h * q.A[2];
  axial_project(x[0][0], x[0][1], x[0][2], r, h, y[0][0], y[0][1], y[0][2]);
  {
    const R yb[3] = {q.Lb[0] + q.sb * h * q.Bz[0], q.Lb[1] + q.sb * h * q.Bz[1], q.Lb[2] + q.sb * h * q.Bz[2]};
    R xa[3];
    axial_project(yb[0], yb[1], yb[2], r, h, xa[0], xa[1], xa[2]);
    np_to_b(q, xa, x[1]);
    np_to_b(q, yb, y[1]);
  }
  {
    const R b = q.A[2], dd = q.la, e = q.L[2];
    const R den = R(1) - b * b;
    R s = den > R(1e-12) ? (b * e - dd) / den : R(0);
    s = g_max1(g_min1(s, h), -h);
    const R t = g_max1(g_min1(b * s + e, h), -h);
    s = g_max1(g_min1(b * t - dd, h), -h);
    const R pa[3] = {q.L[0] + s * q.A[0], q.L[1] + s * q.A[1], q.L[2] + s * q.A[2]};
    const R wx = pa[0], wy = pa[1], wz = pa[2] - t;
    const R wn = g_sqrt(pc_dot(wx, wy, wz, wx, wy, wz));
    const bool ok = far_a && far_b && wn > R(1e-12);
    const R wd = ok ? wn : R(1);
    const R ux = wx / wd, uy = wy / wd, uz = wz / wd;
    const R xq[3] = {pa[0] - r * ux, pa[1] - r * uy, pa[2] - r * uz};
    cyl_project(q.L, q.A, r, h, xq, x[2]);
    axial_project(r * ux, r * uy, t + r * uz, r, h, y[2][0], y[2][1], y[2][2]);
    d[2] = ok ? R(0) : inf;
  }
  for (int c = 0; c < 3; ++c) {
    if (c == 2 && !(d[2] == R(0))) continue;
    const R dx = x[c][0] - y[c][0], dy = x[c][1] - y[c][1], dz = x[c][2] - y[c][2];
    d[c] = g_sqrt(pc_dot(dx, dy, dz, dx, dy, dz));
  }
}
// the least-overlap fallback of bullet_mb.pair_geometry (cores overlapping at every margin level)
template <typename R>
__device__ __forceinline__ void np_fallback(const R ca[3], const R aa[3], const R cb[3], const R ab[3], R r, R hh,
                                            R n[3], R& dist) {
  const R lx = ca[0] - cb[0], ly = ca[1] - cb[1], lz = ca[2] - cb[2];
  const R c2 = pc_dot(lx, ly, lz, lx, ly, lz);
  R best = R(0);
  bool have = false;
  for (int u = 0; u < 3; ++u) {
    R ux, uy, uz;
    if (u == 0) {
      if (!(c2 > R(1e-24))) continue;
      const R l = g_sqrt(c2);
      ux = lx / l; uy = ly / l; uz = lz / l;
    } else {
      const R* a = u == 1 ? aa : ab;
      ux = a[0]; uy = a[1]; uz = a[2];
    }
    if (pc_dot(ux, uy, uz, lx, ly, lz) < R(0)) { ux = -ux; uy = -uy; uz = -uz; }
    const R ov = (cyl_extent_cos(pc_dot(ux, uy, uz, aa[0], aa[1], aa[2]), r, hh) +
                  cyl_extent_cos(pc_dot(ux, uy, uz, ab[0], ab[1], ab[2]), r, hh)) -
                 pc_dot(ux, uy, uz, lx, ly, lz);
    if (!have || ov < best) {
      have = true;
      best = ov;
      n[0] = ux; n[1] = uy; n[2] = uz;
    }
  }
  dist = -best;
}
// bullet_mb.face_points: the face manifold of a cap-to-cap contact - four points spanning the
// overlap of the two near caps (the lens's tips on the line of the cap centres and its corners),
// each carried along n to B's and A's cap planes: point on B fp[k] and distance fd[k]; returns
// false (no points) unless the caps face each other and overlap.
template <typename R>
__device__ __forceinline__ bool face_points(const R ca[3], const R aa[3], const R cb[3], const R ab[3], const R n[3],
                                            R radius, R half_height, R mg, R fp[4][3], R fd[4]) {
  const R r = radius - mg, h = half_height - mg;
  const R sa = pc_dot(cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2], aa[0], aa[1], aa[2]) >= R(0) ? R(1) : R(-1);
  const R sb = pc_dot(ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2], ab[0], ab[1], ab[2]) >= R(0) ? R(1) : R(-1);
  const R nuA[3] = {sa * aa[0], sa * aa[1], sa * aa[2]}, nuB[3] = {sb * ab[0], sb * ab[1], sb * ab[2]};
  const R cB[3] = {cb[0] + sb * h * ab[0], cb[1] + sb * h * ab[1], cb[2] + sb * h * ab[2]};
  const R cab[3] = {(ca[0] + sa * h * aa[0]) - cB[0], (ca[1] + sa * h * aa[1]) - cB[1], (ca[2] + sa * h * aa[2]) - cB[2]};
  const R nb = pc_dot(n[0], n[1], n[2], nuB[0], nuB[1], nuB[2]), na = -pc_dot(n[0], n[1], n[2], nuA[0], nuA[1], nuA[2]);
  const R kf = R(0.7071067811865475244008443621048490);   // FACE_COS
  const R cn = pc_dot(cab[0], cab[1], cab[2], n[0], n[1], n[2]);
  const R dl[3] = {cab[0] - cn * n[0], cab[1] - cn * n[1], cab[2] - cn * n[2]};
  const R s2 = pc_dot(dl[0], dl[1], dl[2], dl[0], dl[1], dl[2]);
  if (!(nb >= kf && na >= kf && s2 < R(4) * r * r)) return false;
  const R s = g_sqrt(s2);
  R u[3];
  if (s > R(1e-9)) {
    u[0] = dl[0] / s; u[1] = dl[1] / s; u[2] = dl[2] / s;
  } else {
    R t2[3];
    plane_space(n, u, t2);
  }
  const R v[3] = {n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]};
  const R w2 = r * r - R(0.25) * s2;
  const R w = g_sqrt(w2 > R(0) ? w2 : R(0));
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const R cu = k == 0 ? s - r : (k == 1 ? r : R(0.5) * s);
    const R cv = k == 2 ? w : (k == 3 ? -w : R(0));
    const R p0 = cu * u[0] + cv * v[0], p1 = cu * u[1] + cv * v[1], p2 = cu * u[2] + cv * v[2];
    const R tb = -pc_dot(p0, p1, p2, nuB[0], nuB[1], nuB[2]) / nb;
    const R ta = pc_dot(cab[0] - p0, cab[1] - p1, cab[2] - p2, nuA[0], nuA[1], nuA[2]) / -na;
    const R tm = tb + mg;
    fp[k][0] = cB[0] + p0 + tm * n[0]; fp[k][1] = cB[1] + p1 + tm * n[1]; fp[k][2] = cB[2] + p2 + tm * n[2];
    fd[k] = (ta - tb) - R(2) * mg;
  }
  return true;
}
// bullet_mb.manifold_replace (btPersistentManifold::sortCachedPoints): the slot of the full cache
// (the four face points: point on B fp, distance fd) the closest point (pb, dist) replaces - never
// a cached point deeper than it, else the slot whose replacement spans the largest quad (Bullet's
// pairing of the cached points on A), the first of a tie; the ties (depth, area) keep rounding
// from deciding a symmetric manifold
template <typename R> struct MfTol;
template <> struct MfTol<double> { static constexpr double depth = 1e-6, area = 1e-4; };   // MANIFOLD_*_TIE
template <> struct MfTol<float> { static constexpr float depth = 1e-6f, area = 1e-4f; };
template <typename R>
__device__ __forceinline__ int manifold_replace(const R pb[3], R dist, const R n[3], const R fp[4][3], const R fd[4]) {
  const R nw[3] = {pb[0] + n[0] * dist, pb[1] + n[1] * dist, pb[2] + n[2] * dist};
  R ca[4][3];
  R maxpen = dist;
  int imax = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ca[k][0] = fp[k][0] + n[0] * fd[k]; ca[k][1] = fp[k][1] + n[1] * fd[k]; ca[k][2] = fp[k][2] + n[2] * fd[k];
    if (fd[k] < maxpen - MfTol<R>::depth) { maxpen = fd[k]; imax = k; }
  }
  R res[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {   // res_k = |(new - c_a) x (c_b - c_c)|^2, (a, b, c) = (1,3,2) (0,3,2) (0,3,1) (0,2,1)
    const int a = k == 0 ? 1 : 0, b = k < 3 ? 3 : 2, c = k < 2 ? 2 : 1;
    const R x0 = nw[0] - ca[a][0], x1 = nw[1] - ca[a][1], x2 = nw[2] - ca[a][2];
    const R y0 = ca[b][0] - ca[c][0], y1 = ca[b][1] - ca[c][1], y2 = ca[b][2] - ca[c][2];
    const R z0 = x1 * y2 - x2 * y1, z1 = x2 * y0 - x0 * y2, z2 = x0 * y1 - x1 * y0;
    res[k] = k == imax ? R(0) : pc_dot(z0, z1, z2, z0, z1, z2);
  }
  const R top = g_max1(g_max1(res[0], res[1]), g_max1(res[2], res[3])) * (R(1) - MfTol<R>::area);
  return res[0] >= top ? 0 : (res[1] >= top ? 1 : (res[2] >= top ? 2 : 3));
}

}  // namespace gpd
