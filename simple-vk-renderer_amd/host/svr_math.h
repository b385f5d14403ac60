// svr_math.h — the handful of GLM calls the reference's host code makes around the draw path, restated
// in fp32 with GLM 0.9.9's scalar operation order (glm is an un-vendored, unpinned submodule of the
// reference).  Call sites restated: update_scene (src/vk_engine.cpp:1492-1495),
// Camera (src/camera.cpp:54-66), node TRS (src/vk_loader.cpp:397-412), MeshNode::Draw (:1717).
// Column-major like glm::mat4: m[c][r].
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace svrm {

struct vec3 {
  float x = 0, y = 0, z = 0;
};
struct vec4 {
  float x = 0, y = 0, z = 0, w = 0;
};
struct quat {  // glm::quat(w, x, y, z)
  float w = 1, x = 0, y = 0, z = 0;
};
struct mat4 {
  float m[4][4];
  float* data() { return &m[0][0]; }
  const float* data() const { return &m[0][0]; }
};

inline mat4 identity() {
  mat4 r;
  std::memset(&r, 0, sizeof(r));
  r.m[0][0] = r.m[1][1] = r.m[2][2] = r.m[3][3] = 1.0f;
  return r;
}
inline float radians(float deg) { return deg * 0.01745329251994329576923690768489f; }

// glm::operator*(mat4, mat4): column j = ((A0*b0 + A1*b1) + A2*b2) + A3*b3
inline mat4 mul(const mat4& a, const mat4& b) {
  mat4 r;
  for (int j = 0; j < 4; j++)
    for (int k = 0; k < 4; k++) {
      float acc = a.m[0][k] * b.m[j][0];
      acc = acc + a.m[1][k] * b.m[j][1];
      acc = acc + a.m[2][k] * b.m[j][2];
      acc = acc + a.m[3][k] * b.m[j][3];
      r.m[j][k] = acc;
    }
  return r;
}
// glm::operator*(mat4, vec4) = (m0*v0 + m1*v1) + (m2*v2 + m3*v3)
inline vec4 mul(const mat4& m, const vec4& v) {
  float o[4];
  for (int k = 0; k < 4; k++) o[k] = (m.m[0][k] * v.x + m.m[1][k] * v.y) + (m.m[2][k] * v.z + m.m[3][k] * v.w);
  return vec4{o[0], o[1], o[2], o[3]};
}
// glm::perspectiveRH_ZO (GLM_FORCE_DEPTH_ZERO_TO_ONE, src/vk_engine.cpp:5)
inline mat4 perspective(float fovy, float aspect, float z_near, float z_far) {
  float tan_half = std::tan(fovy / 2.0f);
  mat4 r;
  std::memset(&r, 0, sizeof(r));
  r.m[0][0] = 1.0f / (aspect * tan_half);
  r.m[1][1] = 1.0f / tan_half;
  r.m[2][2] = z_far / (z_near - z_far);
  r.m[2][3] = -1.0f;
  r.m[3][2] = -(z_far * z_near) / (z_far - z_near);
  return r;
}
inline mat4 translate(const mat4& m, vec3 v) {
  mat4 r = m;
  for (int k = 0; k < 4; k++) r.m[3][k] = m.m[0][k] * v.x + m.m[1][k] * v.y + m.m[2][k] * v.z + m.m[3][k];
  return r;
}
inline mat4 scale(const mat4& m, vec3 v) {
  mat4 r;
  for (int k = 0; k < 4; k++) {
    r.m[0][k] = m.m[0][k] * v.x;
    r.m[1][k] = m.m[1][k] * v.y;
    r.m[2][k] = m.m[2][k] * v.z;
    r.m[3][k] = m.m[3][k];
  }
  return r;
}
inline quat angle_axis(float angle, vec3 axis) {
  float s = std::sin(angle * 0.5f);
  return quat{std::cos(angle * 0.5f), axis.x * s, axis.y * s, axis.z * s};
}
// glm::toMat4(quat)
inline mat4 to_mat4(quat q) {
  float qxx = q.x * q.x, qyy = q.y * q.y, qzz = q.z * q.z;
  float qxz = q.x * q.z, qxy = q.x * q.y, qyz = q.y * q.z;
  float qwx = q.w * q.x, qwy = q.w * q.y, qwz = q.w * q.z;
  mat4 r = identity();
  r.m[0][0] = 1.0f - 2.0f * (qyy + qzz);
  r.m[0][1] = 2.0f * (qxy + qwz);
  r.m[0][2] = 2.0f * (qxz - qwy);
  r.m[1][0] = 2.0f * (qxy - qwz);
  r.m[1][1] = 1.0f - 2.0f * (qxx + qzz);
  r.m[1][2] = 2.0f * (qyz + qwx);
  r.m[2][0] = 2.0f * (qxz + qwy);
  r.m[2][1] = 2.0f * (qyz - qwx);
  r.m[2][2] = 1.0f - 2.0f * (qxx + qyy);
  return r;
}
// glm::inverse(mat4): cofactor expansion (detail::compute_inverse<4,4>)
inline mat4 inverse(const mat4& mm) {
  const float(*m)[4] = mm.m;
  float c00 = m[2][2] * m[3][3] - m[3][2] * m[2][3], c02 = m[1][2] * m[3][3] - m[3][2] * m[1][3];
  float c03 = m[1][2] * m[2][3] - m[2][2] * m[1][3], c04 = m[2][1] * m[3][3] - m[3][1] * m[2][3];
  float c06 = m[1][1] * m[3][3] - m[3][1] * m[1][3], c07 = m[1][1] * m[2][3] - m[2][1] * m[1][3];
  float c08 = m[2][1] * m[3][2] - m[3][1] * m[2][2], c10 = m[1][1] * m[3][2] - m[3][1] * m[1][2];
  float c11 = m[1][1] * m[2][2] - m[2][1] * m[1][2], c12 = m[2][0] * m[3][3] - m[3][0] * m[2][3];
  float c14 = m[1][0] * m[3][3] - m[3][0] * m[1][3], c15 = m[1][0] * m[2][3] - m[2][0] * m[1][3];
  float c16 = m[2][0] * m[3][2] - m[3][0] * m[2][2], c18 = m[1][0] * m[3][2] - m[3][0] * m[1][2];
  float c19 = m[1][0] * m[2][2] - m[2][0] * m[1][2], c20 = m[2][0] * m[3][1] - m[3][0] * m[2][1];
  float c22 = m[1][0] * m[3][1] - m[3][0] * m[1][1], c23 = m[1][0] * m[2][1] - m[2][0] * m[1][1];
  float f0[4] = {c00, c00, c02, c03}, f1[4] = {c04, c04, c06, c07}, f2[4] = {c08, c08, c10, c11};
  float f3[4] = {c12, c12, c14, c15}, f4[4] = {c16, c16, c18, c19}, f5[4] = {c20, c20, c22, c23};
  float v0[4] = {m[1][0], m[0][0], m[0][0], m[0][0]}, v1[4] = {m[1][1], m[0][1], m[0][1], m[0][1]};
  float v2[4] = {m[1][2], m[0][2], m[0][2], m[0][2]}, v3[4] = {m[1][3], m[0][3], m[0][3], m[0][3]};
  const float sa[4] = {1, -1, 1, -1}, sb[4] = {-1, 1, -1, 1};
  mat4 inv;
  for (int k = 0; k < 4; k++) {
    float i0 = v1[k] * f0[k] - v2[k] * f1[k] + v3[k] * f2[k];
    float i1 = v0[k] * f0[k] - v2[k] * f3[k] + v3[k] * f4[k];
    float i2 = v0[k] * f1[k] - v1[k] * f3[k] + v3[k] * f5[k];
    float i3 = v0[k] * f2[k] - v1[k] * f4[k] + v2[k] * f5[k];
    inv.m[0][k] = i0 * sa[k];
    inv.m[1][k] = i1 * sb[k];
    inv.m[2][k] = i2 * sa[k];
    inv.m[3][k] = i3 * sb[k];
  }
  float d0 = m[0][0] * inv.m[0][0], d1 = m[0][1] * inv.m[1][0], d2 = m[0][2] * inv.m[2][0], d3 = m[0][3] * inv.m[3][0];
  float one_over_det = 1.0f / ((d0 + d1) + (d2 + d3));
  for (int c = 0; c < 4; c++)
    for (int k = 0; k < 4; k++) inv.m[c][k] = inv.m[c][k] * one_over_det;
  return inv;
}

// ---- temporal antialiasing (include/svr_temporal.h): the caller's side.  glmath.py restates these three; the two agree
// bit for bit (tests/test_jitter.py).
// The i-th element (i >= 1) of the Halton sequence of a base: the radical inverse, accumulated in double, rounded once.
inline float halton(unsigned i, unsigned base) {
  double f = 1.0, r = 0.0;
  while (i > 0u) {
    f = f / (double)base;
    r = r + f * (double)(i % base);
    i /= base;
  }
  return (float)r;
}
// proj with a sub-pixel shift of (jx, jy) pixels in a w x h target: 2 jx / w and 2 jy / h times the w row are added to the
// x and y rows, so a point that landed at pixel (px, py) lands at (px + jx, py + jy).
inline mat4 jitter_projection(const mat4& proj, float jx, float jy, float w, float h) {
  const float ax = (2.0f * jx) / w, ay = (2.0f * jy) / h;
  mat4 r = proj;
  for (int c = 0; c < 4; c++) {
    r.m[c][0] = proj.m[c][0] + ax * proj.m[c][3];
    r.m[c][1] = proj.m[c][1] + ay * proj.m[c][3];
  }
  return r;
}
// SvrTemporalPass.reproject = prev_viewproj * inverse(viewproj), both without jitter: the inverse (the cofactor expansion
// above) and the product are taken in double and rounded to fp32 once.
inline mat4 temporal_reproject(const mat4& prev_viewproj, const mat4& viewproj) {
  double m[4][4], p[4][4], inv[4][4];
  for (int c = 0; c < 4; c++)
    for (int k = 0; k < 4; k++) {
      m[c][k] = (double)viewproj.m[c][k];
      p[c][k] = (double)prev_viewproj.m[c][k];
    }
  double c00 = m[2][2] * m[3][3] - m[3][2] * m[2][3], c02 = m[1][2] * m[3][3] - m[3][2] * m[1][3];
  double c03 = m[1][2] * m[2][3] - m[2][2] * m[1][3], c04 = m[2][1] * m[3][3] - m[3][1] * m[2][3];
  double c06 = m[1][1] * m[3][3] - m[3][1] * m[1][3], c07 = m[1][1] * m[2][3] - m[2][1] * m[1][3];
  double c08 = m[2][1] * m[3][2] - m[3][1] * m[2][2], c10 = m[1][1] * m[3][2] - m[3][1] * m[1][2];
  double c11 = m[1][1] * m[2][2] - m[2][1] * m[1][2], c12 = m[2][0] * m[3][3] - m[3][0] * m[2][3];
  double c14 = m[1][0] * m[3][3] - m[3][0] * m[1][3], c15 = m[1][0] * m[2][3] - m[2][0] * m[1][3];
  double c16 = m[2][0] * m[3][2] - m[3][0] * m[2][2], c18 = m[1][0] * m[3][2] - m[3][0] * m[1][2];
  double c19 = m[1][0] * m[2][2] - m[2][0] * m[1][2], c20 = m[2][0] * m[3][1] - m[3][0] * m[2][1];
  double c22 = m[1][0] * m[3][1] - m[3][0] * m[1][1], c23 = m[1][0] * m[2][1] - m[2][0] * m[1][1];
  double f0[4] = {c00, c00, c02, c03}, f1[4] = {c04, c04, c06, c07}, f2[4] = {c08, c08, c10, c11};
  double f3[4] = {c12, c12, c14, c15}, f4[4] = {c16, c16, c18, c19}, f5[4] = {c20, c20, c22, c23};
  double v0[4] = {m[1][0], m[0][0], m[0][0], m[0][0]}, v1[4] = {m[1][1], m[0][1], m[0][1], m[0][1]};
  double v2[4] = {m[1][2], m[0][2], m[0][2], m[0][2]}, v3[4] = {m[1][3], m[0][3], m[0][3], m[0][3]};
  const double sa[4] = {1, -1, 1, -1}, sb[4] = {-1, 1, -1, 1};
  for (int k = 0; k < 4; k++) {
    inv[0][k] = (v1[k] * f0[k] - v2[k] * f1[k] + v3[k] * f2[k]) * sa[k];
    inv[1][k] = (v0[k] * f0[k] - v2[k] * f3[k] + v3[k] * f4[k]) * sb[k];
    inv[2][k] = (v0[k] * f1[k] - v1[k] * f3[k] + v3[k] * f5[k]) * sa[k];
    inv[3][k] = (v0[k] * f2[k] - v1[k] * f4[k] + v2[k] * f5[k]) * sb[k];
  }
  const double d0 = m[0][0] * inv[0][0], d1 = m[0][1] * inv[1][0], d2 = m[0][2] * inv[2][0], d3 = m[0][3] * inv[3][0];
  const double one_over_det = 1.0 / ((d0 + d1) + (d2 + d3));
  mat4 r;
  for (int j = 0; j < 4; j++) {
    double col[4];
    for (int k = 0; k < 4; k++) col[k] = inv[j][k] * one_over_det;
    for (int k = 0; k < 4; k++) r.m[j][k] = (float)(((p[0][k] * col[0] + p[1][k] * col[1]) + p[2][k] * col[2]) + p[3][k] * col[3]);
  }
  return r;
}

// ---- ambient occlusion (include/svr_ambient.h): the caller's side; glmath.py's pixels_per_unit is the same bit for bit
// (tests/test_ambient_math.py).
// SvrAmbientPass.pixels_per_unit: the pixels one world unit spans at clip w = 1 in a target of the given height.
inline float pixels_per_unit(const mat4& proj, float height) { return (0.5f * height) * std::fabs(proj.m[1][1]); }

// ---- the upscaled present (include/svr_upscale.h): the caller's side; glmath.py's render_extent is the same
// The extent a frame is rendered at under a render scale: the reference's expression (src/vk_engine.cpp:1220-1222), a float
// product truncated to uint32, each way; at least 1.
inline void render_extent(uint32_t window_w, uint32_t window_h, float scale, uint32_t* w, uint32_t* h) {
  const uint32_t rw = (uint32_t)((float)window_w * scale), rh = (uint32_t)((float)window_h * scale);
  *w = rw < 1u ? 1u : rw;
  *h = rh < 1u ? 1u : rh;
}

// ---- the depth of field pass (include/svr_dof.h): the caller's side; glmath.py's dof_depth_terms and dof_blur_scale are
// the same bit for bit (tests/test_dof_ref.py states them, tests/test_host_cpp_dof.py compares the two).
// SvrDofPass.inv_z_scale and inv_z_bias of a perspective projection, jittered or not: 1 / view distance =
// depth * scale + bias, with depth = (proj[2][2] z + proj[3][2]) / -z.  Taken in double, rounded once each.
inline void dof_depth_terms(const mat4& proj, float* inv_z_scale, float* inv_z_bias) {
  const double b = (double)proj.m[3][2];
  *inv_z_scale = (float)(1.0 / b);
  *inv_z_bias = (float)((double)proj.m[2][2] / b);
}
// SvrDofPass.blur_scale of a thin lens: the radius, in pixels of a target of the given height, of the circle of confusion
// of a point at infinity, 0.5 f^2 / (N (zf - f)) scaled from the sensor to the target.  Taken in double, rounded once.
inline float dof_blur_scale(float focal_length, float f_number, float focus_distance, float sensor_height, float target_height) {
  const double f = focal_length, n = f_number, zf = focus_distance, sh = sensor_height, th = target_height;
  return (float)(((0.5 * f * f) / (n * (zf - f))) * th / sh);
}

}  // namespace svrm
