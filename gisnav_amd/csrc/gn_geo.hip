// Post-pose georeferencing of GISNav's PoseNode, host-side scalar code:
// camera position in the reference raster -> WGS 84 -> ECEF, orientation -> ENU -> ECEF quaternion.
//   ros/gisnav/gisnav/core/pose_node.py:333-381, ros/gisnav/gisnav/_transformations.py:298-393
// (pyproj `latlong -> geocent` on the WGS 84 datum and transforms3d `mat2quat` are restated in closed form).
#include "gn_common.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

namespace {
constexpr double kA = 6378137.0;                    // WGS 84 semi-major axis
constexpr double kF = 1.0 / 298.257223563;          // WGS 84 flattening
constexpr double kPi = 3.14159265358979323846;

// symmetric 4x4 eigen-decomposition by cyclic Jacobi; returns the eigenvector of the largest eigenvalue
void top_eigenvector4(double K[4][4], double q[4]) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0;
    for (int p = 0; p < 4; ++p) for (int r = p + 1; r < 4; ++r) off += K[p][r] * K[p][r];
    if (off < 1e-300) break;
    for (int p = 0; p < 4; ++p)
      for (int r = p + 1; r < 4; ++r) {
        if (K[p][r] == 0.0) continue;
        const double theta = (K[r][r] - K[p][p]) / (2.0 * K[p][r]);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 4; ++k) { const double kp = K[k][p], kr = K[k][r]; K[k][p] = c * kp - s * kr; K[k][r] = s * kp + c * kr; }
        for (int k = 0; k < 4; ++k) { const double pk = K[p][k], rk = K[r][k]; K[p][k] = c * pk - s * rk; K[r][k] = s * pk + c * rk; }
        for (int k = 0; k < 4; ++k) { const double vp = V[k][p], vr = V[k][r]; V[k][p] = c * vp - s * vr; V[k][r] = s * vp + c * vr; }
      }
  }
  int best = 0;
  for (int i = 1; i < 4; ++i) if (K[i][i] > K[best][best]) best = i;
  for (int k = 0; k < 4; ++k) q[k] = V[k][best];
}

// pose_node.py:345-381 behind the range check: camera centre `pos` (raster coordinates) and r_inv = R_wc through the raster's affine CRS ->
// WGS 84, ECEF position and ECEF orientation quaternion (x, y, z, w).  gn_pose_to_earth's map; gn_pose_cov_to_earth differentiates it.
void camera_to_earth(const double pos[3], const double ri[3][3], const double* affine12, double* position_ecef3, double* quat_xyzw4, double* lonlatalt3) {
  double w84[3];                                      // t_wgs84 = affine @ [pos; 1]
  for (int i = 0; i < 3; ++i) w84[i] = affine12[4 * i] * pos[0] + affine12[4 * i + 1] * pos[1] + affine12[4 * i + 2] * pos[2] + affine12[4 * i + 3];
  if (lonlatalt3) { lonlatalt3[0] = w84[0]; lonlatalt3[1] = w84[1]; lonlatalt3[2] = w84[2]; }
  gn_wgs84_to_ecef(w84[0], w84[1], w84[2], position_ecef3);
  double Rn[3][3];                                    // R = affine[:3, :3] / column norms
  for (int j = 0; j < 3; ++j) {
    const double n = std::sqrt(affine12[j] * affine12[j] + affine12[4 + j] * affine12[4 + j] + affine12[8 + j] * affine12[8 + j]);
    for (int i = 0; i < 3; ++i) Rn[i][j] = affine12[4 * i + j] / n;
  }
  double enu[3][3];                                   // camera_optical_rotation_in_enu = R @ r_inv
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) enu[i][j] = Rn[i][0] * ri[0][j] + Rn[i][1] * ri[1][j] + Rn[i][2] * ri[2][j];
  const double lon = w84[0] * (kPi / 180.0), lat = w84[1] * (kPi / 180.0);     // enu_to_ecef_matrix(lon, lat)
  const double slat = std::sin(lat), clat = std::cos(lat), slon = std::sin(lon), clon = std::cos(lon);
  const double E[3][3] = {{-slon, -slat * clon, clat * clon}, {clon, -slat * slon, clat * slon}, {0, clat, slat}};
  double M[3][3];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) M[i][j] = E[i][0] * enu[0][j] + E[i][1] * enu[1][j] + E[i][2] * enu[2][j];
  // transforms3d.quaternions.mat2quat: eigenvector of the largest eigenvalue of K, w >= 0; tf_transformations order x, y, z, w
  const double Qxx = M[0][0], Qyx = M[0][1], Qzx = M[0][2], Qxy = M[1][0], Qyy = M[1][1], Qzy = M[1][2], Qxz = M[2][0], Qyz = M[2][1], Qzz = M[2][2];
  double K[4][4] = {{Qxx - Qyy - Qzz, Qyx + Qxy, Qzx + Qxz, Qyz - Qzy},
                    {Qyx + Qxy, Qyy - Qxx - Qzz, Qzy + Qyz, Qzx - Qxz},
                    {Qzx + Qxz, Qzy + Qyz, Qzz - Qxx - Qyy, Qxy - Qyx},
                    {Qyz - Qzy, Qzx - Qxz, Qxy - Qyx, Qxx + Qyy + Qzz}};
  for (auto& row : K) for (double& v : row) v /= 3.0;
  double q[4];
  top_eigenvector4(K, q);                              // (x, y, z, w)
  const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sgn = q[3] < 0 ? -1.0 : 1.0;
  for (int k = 0; k < 4; ++k) quat_xyzw4[k] = sgn * q[k] / nq;
}

// r_inv = r.T, camera_optical_position_in_world = -r_inv @ t, and pose_node.py:339-341's range test (the reference compares x with shape[0],
// y with shape[1]; int(x) truncates toward zero)
bool camera_in_raster(const double* R9, const double* t3, int ref_h, int ref_w, double ri[3][3], double pos[3]) {
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) ri[i][j] = R9[j * 3 + i];
  for (int i = 0; i < 3; ++i) pos[i] = -(ri[i][0] * t3[0] + ri[i][1] * t3[1] + ri[i][2] * t3[2]);
  const long long xi = (long long)pos[0], yi = (long long)pos[1];
  return 0 <= xi && xi <= ref_h && 0 <= yi && yi <= ref_w;
}

void skew3(const double v[3], double S[3][3]) {
  S[0][0] = 0; S[0][1] = -v[2]; S[0][2] = v[1]; S[1][0] = v[2]; S[1][1] = 0; S[1][2] = -v[0]; S[2][0] = -v[1]; S[2][1] = v[0]; S[2][2] = 0;
}
void matmul3(const double A[3][3], const double B[3][3], double C[3][3]) {
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) C[i][j] = A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j];
}
// Exp(w) of SO(3) (Rodrigues' formula)
void so3_exp(const double w[3], double R[3][3]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
  const double a = th < 1e-4 ? 1.0 - th2 / 6.0 : std::sin(th) / th, b = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - std::cos(th)) / th2;
  double S[3][3], S2[3][3];
  skew3(w, S); matmul3(S, S, S2);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[i][j] = (i == j ? 1.0 : 0.0) + a * S[i][j] + b * S2[i][j];
}
// rotation vector of a rotation matrix, through the unit quaternion (Shepperd's branch on the largest of w, x, y, z: accurate at every angle)
void so3_log(const double R[3][3], double w[3]) {
  const double tr = R[0][0] + R[1][1] + R[2][2];
  double q[4];                                          // (w, x, y, z) up to scale
  if (tr > 0) { q[0] = 1.0 + tr; q[1] = R[2][1] - R[1][2]; q[2] = R[0][2] - R[2][0]; q[3] = R[1][0] - R[0][1]; }
  else if (R[0][0] >= R[1][1] && R[0][0] >= R[2][2]) { q[0] = R[2][1] - R[1][2]; q[1] = 1.0 + R[0][0] - R[1][1] - R[2][2]; q[2] = R[0][1] + R[1][0]; q[3] = R[0][2] + R[2][0]; }
  else if (R[1][1] >= R[2][2]) { q[0] = R[0][2] - R[2][0]; q[1] = R[0][1] + R[1][0]; q[2] = 1.0 + R[1][1] - R[0][0] - R[2][2]; q[3] = R[1][2] + R[2][1]; }
  else { q[0] = R[1][0] - R[0][1]; q[1] = R[0][2] + R[2][0]; q[2] = R[1][2] + R[2][1]; q[3] = 1.0 + R[2][2] - R[0][0] - R[1][1]; }
  if (q[0] < 0) for (double& v : q) v = -v;
  const double vn = std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double k = vn < 1e-12 * q[0] ? 2.0 / q[0] : 2.0 * std::atan2(vn, q[0]) / vn;      // angle / |v|
  for (int i = 0; i < 3; ++i) w[i] = k * q[1 + i];
}
// C = J S J^T for 6x6 row-major matrices, symmetrised
void congruence6(const double J[6][6], const double* S36, double* C36) {
  double T[6][6];
  for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) { double a = 0; for (int k = 0; k < 6; ++k) a += J[i][k] * S36[6 * k + j]; T[i][j] = a; }
  double C[6][6];
  for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) { double a = 0; for (int k = 0; k < 6; ++k) a += T[i][k] * J[j][k]; C[i][j] = a; }
  for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) C36[6 * i + j] = 0.5 * (C[i][j] + C[j][i]);
}
// d(c, phi) / d(rvec, tvec) at (R, t): c = -R^T t, R_wc,true = Exp(phi) R_wc.  R(r + dr) = R Exp(J_r(r) dr) with the right Jacobian
// J_r = I - (1 - cos th) / th^2 [r]x + (th - sin th) / th^3 [r]x^2, so phi = -J_r dr and dc = -R^T dt - [c]x phi.
void camera_jacobian(const double* R9, const double* t3, double A[6][6]) {
  double R[3][3], r[3], c[3];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[i][j] = R9[3 * i + j];
  so3_log(R, r);
  for (int i = 0; i < 3; ++i) c[i] = -(R[0][i] * t3[0] + R[1][i] * t3[1] + R[2][i] * t3[2]);
  const double th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2], th = std::sqrt(th2);
  const double a = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - std::cos(th)) / th2, b = th < 1e-4 ? 1.0 / 6.0 - th2 / 120.0 : (th - std::sin(th)) / (th2 * th);
  double S[3][3], S2[3][3], Jr[3][3], Cx[3][3], CJ[3][3];
  skew3(r, S); matmul3(S, S, S2);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Jr[i][j] = (i == j ? 1.0 : 0.0) - a * S[i][j] + b * S2[i][j];
  skew3(c, Cx); matmul3(Cx, Jr, CJ);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { A[i][j] = CJ[i][j]; A[i][3 + j] = -R[j][i]; A[3 + i][j] = -Jr[i][j]; A[3 + i][3 + j] = 0.0; }
}
}  // namespace

extern "C" {

// _transformations.py:298-323 proj_to_affine: "+proj=affine +xoff=.. +yoff=.. +zoff=.. +s11=.. ... +s33=.." -> 3x4 row-major
int gn_proj_to_affine(const char* proj_str, double* affine12) {
  if (!proj_str || !affine12) return GN_ERR_ARG;
  static const char* keys[12] = {"+s11", "+s12", "+s13", "+xoff", "+s21", "+s22", "+s23", "+yoff", "+s31", "+s32", "+s33", "+zoff"};
  const std::string s(proj_str);
  for (int i = 0; i < 12; ++i) {
    const std::string key = std::string(keys[i]) + "=";
    size_t pos = 0; bool found = false;
    while ((pos = s.find(key, pos)) != std::string::npos) {
      if (pos == 0 || s[pos - 1] == ' ') { found = true; break; }      // whole token, as str.split() sees it
      pos += key.size();
    }
    if (!found) return GN_ERR_NAME;
    char* end = nullptr;
    const char* start = s.c_str() + pos + key.size();
    affine12[i] = std::strtod(start, &end);
    if (end == start) return GN_ERR_NAME;
  }
  return GN_OK;
}

// _transformations.py:326-345 wgs84_to_ecef (pyproj latlong -> geocent, WGS 84): closed form
int gn_wgs84_to_ecef(double lon_deg, double lat_deg, double alt, double* xyz3) {
  if (!xyz3) return GN_ERR_ARG;
  const double lon = lon_deg * (kPi / 180.0), lat = lat_deg * (kPi / 180.0);
  const double e2 = kF * (2.0 - kF);
  const double sl = std::sin(lat), cl = std::cos(lat);
  const double N = kA / std::sqrt(1.0 - e2 * sl * sl);
  xyz3[0] = (N + alt) * cl * std::cos(lon);
  xyz3[1] = (N + alt) * cl * std::sin(lon);
  xyz3[2] = (N * (1.0 - e2) + alt) * sl;
  return GN_OK;
}

// pose_node.py:333-381: (r, t) of compute_pose + the raster's affine CRS -> earth-frame position and orientation.
// Returns GN_OK, or 1 when the camera centre falls outside the expected range of the reference raster (the node logs a
// warning and returns None, pose_node.py:339-341).
int gn_pose_to_earth(const double* R9, const double* t3, const double* affine12, int ref_h, int ref_w,
                     double* position_ecef3, double* quat_xyzw4, double* lonlatalt3) {
  if (!R9 || !t3 || !affine12 || !position_ecef3 || !quat_xyzw4) return GN_ERR_ARG;
  double ri[3][3], pos[3];
  if (!camera_in_raster(R9, t3, ref_h, ref_w, ri, pos)) return 1;
  camera_to_earth(pos, ri, affine12, position_ecef3, quat_xyzw4, lonlatalt3);
  return GN_OK;
}

// Covariance of (rvec, tvec) -> covariance of (c, phi): camera centre c = -R^T t in raster coordinates and the rotation increment of
// R_wc = R^T, R_wc,true = Exp(phi) R_wc (closed form, DESIGN.md "Pose covariance").  Order (cx, cy, cz, phi_x, phi_y, phi_z), raster px / rad.
int gn_pose_cov_to_camera(const double* R9, const double* t3, const double* cov_rt36, double* cov_cam36) {
  if (!R9 || !t3 || !cov_rt36 || !cov_cam36) return GN_ERR_ARG;
  double A[6][6];
  camera_jacobian(R9, t3, A);
  congruence6(A, cov_rt36, cov_cam36);
  return GN_OK;
}

// The same covariance pushed through gn_pose_to_earth's map: order (ECEF x, y, z [m], psi_x, psi_y, psi_z [rad]) with q_true = dq(psi) (x) q_est for
// the quaternion gn_pose_to_earth returns -- rotation about the fixed ECEF axes, the layout of geometry_msgs/PoseWithCovariance.  The map
// normalises the affine's columns (not orthogonal for a rotated lon / lat grid) and takes the quaternion by the eigenvector method, so its Jacobian
// is DEFINED by the map: central differences of camera_to_earth over the six tangent directions of (c, phi).  Steps 1e-2 px / 1e-5 rad: truncation
// ~ step^2 (the map is smooth at the scale of the earth's radius / of a radian), rounding ~ 1e-16 * 6.4e6 m / 2e-2 px = 3e-8 relative for the
// position and 1e-16 / 2e-5 = 5e-12 for the orientation.  Returns 1 exactly where gn_pose_to_earth does (cov_earth36 is then left untouched).
int gn_pose_cov_to_earth(const double* R9, const double* t3, const double* cov_rt36, const double* affine12, int ref_h, int ref_w,
                         double* cov_earth36) {
  if (!R9 || !t3 || !cov_rt36 || !affine12 || !cov_earth36) return GN_ERR_ARG;
  double ri[3][3], pos[3];
  if (!camera_in_raster(R9, t3, ref_h, ref_w, ri, pos)) return 1;
  double A[6][6], cov_cam[36], J[6][6];
  camera_jacobian(R9, t3, A);
  congruence6(A, cov_rt36, cov_cam);
  for (int k = 0; k < 6; ++k) {
    const double h = k < 3 ? 1e-2 : 1e-5;
    double p[2][3], q[2][4];
    for (int side = 0; side < 2; ++side) {
      const double d = side == 0 ? h : -h;
      double c[3] = {pos[0], pos[1], pos[2]}, Rw[3][3];
      if (k < 3) {
        c[k] += d;
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rw[i][j] = ri[i][j];
      } else {
        double w[3] = {0, 0, 0}, E[3][3];
        w[k - 3] = d;
        so3_exp(w, E); matmul3(E, ri, Rw);
      }
      camera_to_earth(c, Rw, affine12, p[side], q[side], nullptr);
    }
    // dq = q+ (x) conj(q-) = (cos(|psi|), sin(|psi|) psi / |psi|) for the rotation 2 psi between the two sides
    const double *a = q[0], *b = q[1];
    double dq[4] = {-a[3] * b[0] + a[0] * b[3] - a[1] * b[2] + a[2] * b[1], -a[3] * b[1] + a[0] * b[2] + a[1] * b[3] - a[2] * b[0],
                    -a[3] * b[2] - a[0] * b[1] + a[1] * b[0] + a[2] * b[3], a[3] * b[3] + a[0] * b[0] + a[1] * b[1] + a[2] * b[2]};
    if (dq[3] < 0) for (double& v : dq) v = -v;         // (q and -q are one rotation: the w >= 0 convention may flip between the sides)
    const double vn = std::sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2]);
    const double ang = vn > 0 ? 2.0 * std::atan2(vn, dq[3]) / vn : 2.0;
    for (int i = 0; i < 3; ++i) { J[i][k] = (p[0][i] - p[1][i]) / (2.0 * h); J[3 + i][k] = ang * dq[i] / (2.0 * h); }
  }
  congruence6(J, cov_cam, cov_earth36);
  return GN_OK;
}

}  // extern "C"
