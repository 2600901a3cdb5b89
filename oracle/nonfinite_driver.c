/*
 * nonfinite_driver.c -- stand-alone driver of the oracle for sanitizer builds (`make -C oracle san`).
 *
 * TEST INFRASTRUCTURE ONLY.  Includes gsr_oracle.c, renders a small LCG-random scene forward (both binning modes) and
 * backward, once clean and once with NaN / +Inf / -Inf written into every input field of a few rows, and prints a
 * checksum of the integer stages.  Built with -fsanitize=address,undefined it shows that no non-finite input makes the
 * oracle convert an unrepresentable float, index outside a buffer or read an uninitialised instance.
 */
#include "gsr_oracle.c"

#include <stdio.h>

static uint32_t lcg_state = 12345u;
static float rnd(void) { /* [0, 1) */
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return (float)(lcg_state >> 8) * (1.0f / 16777216.0f);
}

int main(void) {
  enum { P = 300, W = 65, H = 49, M = 16 };
  static float means[P * 3], scales[P * 3], rots[P * 4], opac[P], shs[P * M * 3], cov[P * 6], col[P * 3];
  const float tanx = 0.57735026f, tany = tanx * H / W, zn = 0.01f, zf = 100.0f;
  float view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, proj[16] = {0}, cam[3] = {0, 0, 0}, bg[3] = {1, 1, 1};
  proj[0] = 1.0f / tanx; proj[5] = 1.0f / tany; proj[10] = zf / (zf - zn); proj[11] = 1.0f; proj[14] = -(zf * zn) / (zf - zn);
  static float dpix[3 * H * W], dacc[H * W];
  for (int i = 0; i < 3 * H * W; i++) dpix[i] = rnd() - 0.5f;
  for (int i = 0; i < H * W; i++) dacc[i] = rnd() - 0.5f;
  const float poison[3] = {NAN, INFINITY, -INFINITY};
  unsigned long long sum = 0;
  for (int pass = 0; pass < 1 + 3 * 7; pass++) { /* clean, then value x field */
    for (int i = 0; i < P; i++) {
      float z = 1.0f + 8.0f * rnd();
      means[3 * i] = (2 * rnd() - 1) * z * tanx; means[3 * i + 1] = (2 * rnd() - 1) * z * tany; means[3 * i + 2] = z;
      float n = 0;
      for (int k = 0; k < 4; k++) { rots[4 * i + k] = 2 * rnd() - 1; n += rots[4 * i + k] * rots[4 * i + k]; }
      for (int k = 0; k < 4; k++) rots[4 * i + k] /= sqrtf(n);
      for (int k = 0; k < 3; k++) { scales[3 * i + k] = 0.004f + 0.2f * rnd(); col[3 * i + k] = rnd(); }
      opac[i] = 0.05f + 0.9f * rnd();
      for (int k = 0; k < M * 3; k++) shs[i * M * 3 + k] = (k < 3 ? 3.0f : 0.2f) * (rnd() - 0.5f);
      for (int k = 0; k < 6; k++) cov[6 * i + k] = (k == 0 || k == 3 || k == 5) ? 0.001f + 0.01f * rnd() : 0.0f;
    }
    const int field = pass ? (pass - 1) % 7 : -1;
    if (pass)
      for (int r = 0; r < P; r += (r == 0 ? 255 : r == 255 ? 1 : 43)) {
        const float v = poison[(pass - 1) / 7];
        float* dst[7] = {&means[3 * r], &means[3 * r + 2], &scales[3 * r + 1], &rots[4 * r + 2], &opac[r],
                         &shs[r * M * 3 + 28], &cov[6 * r + 3]};
        *dst[field] = v;
        if (field == 5) col[3 * r + 1] = v;
      }
    for (int route = 0; route < 2; route++) /* scales + rotations + SH, then precomputed covariance + colour */
      for (int tight = 0; tight < 2; tight++) {
        gsro_set_tight(tight);
        gsro_frame* f = gsro_forward(P, 3, M, bg, W, H, means, route ? NULL : shs, route ? col : NULL, opac,
                                     route ? NULL : scales, 1.0f, route ? NULL : rots, route ? cov : NULL, view, proj, cam,
                                     tanx, tany);
        static float g2[P * 3], gc[P * 4], go[P], gcol[P * 3], g3[P * 3], gcov[P * 6], gsh[P * M * 3], gs[P * 3], gr[P * 4];
        memset(g2, 0, sizeof g2); memset(gc, 0, sizeof gc); memset(go, 0, sizeof go); memset(gcol, 0, sizeof gcol);
        memset(g3, 0, sizeof g3); memset(gcov, 0, sizeof gcov); memset(gsh, 0, sizeof gsh); memset(gs, 0, sizeof gs);
        memset(gr, 0, sizeof gr);
        gsro_backward(f, bg, means, route ? NULL : shs, route ? col : NULL, route ? NULL : scales, 1.0f,
                      route ? NULL : rots, route ? cov : NULL, view, proj, cam, tanx, tany, dpix, dacc, g2, gc, go, gcol, g3,
                      gcov, gsh, gs, gr);
        sum = sum * 1000003ull + (unsigned long long)f->R;
        for (int i = 0; i < P; i++) sum = sum * 31ull + (unsigned long long)(unsigned)f->radii[i] + f->tiles_touched[i];
        for (int i = 0; i < f->R; i++) sum = sum * 31ull + f->point_list[i];
        gsro_free(f);
      }
  }
  gsro_set_tight(0);
  printf("nonfinite_driver ok: checksum %llu\n", sum);
  return 0;
}
