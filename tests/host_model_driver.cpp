// host_model_driver.cpp — stand-alone checks of csrc/gpd_host_model.h, the HIP-free host model of
// libgpd.so, built with a plain C++ compiler under AddressSanitizer + UBSan (tests/test_host_model.py).
// Inside the library this code runs only while a sim is created or its tables are replaced, that is
// with a GPU; here it runs without one.  Prints OK and exits 0, or one FAIL line per broken check.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../gym_pybullet_drones_routing_amd/csrc/gpd_host_model.h"

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                                    \
    }                                                                \
  } while (0)

int main() {
  // pose_tables: one set of three drones with zero rpy
  const int D = 3;
  const double xyz[D * 3] = {0.0, 0.0, 0.1125, 0.1588, 0.1588, 0.1125, -0.3, 0.25, 2.0};
  const double zero[D * 3] = {};
  std::vector<double> tmpl(D * 10), tgt(D * 3);
  pose_tables(GPD_TASK_MULTIHOVER, 1, D, xyz, zero, tmpl.data(), tgt.data());
  for (int d = 0; d < D; ++d) {
    const double* t = &tmpl[d * 10];
    const double want[10] = {xyz[d * 3], xyz[d * 3 + 1], xyz[d * 3 + 2], 0, 0, 0, 1, 0, 0, 0};
    for (int k = 0; k < 10; ++k) CHECK(t[k] == want[k]);
    CHECK(tgt[d * 3] == xyz[d * 3] && tgt[d * 3 + 1] == xyz[d * 3 + 1]);
    CHECK(tgt[d * 3 + 2] == xyz[d * 3 + 2] + 1.0 / (d + 1));
  }
  pose_tables(GPD_TASK_HOVER, 1, D, xyz, zero, tmpl.data(), tgt.data());
  for (int d = 0; d < D; ++d) CHECK(tgt[d * 3] == 0.0 && tgt[d * 3 + 1] == 0.0 && tgt[d * 3 + 2] == 1.0);

  // pose_template: pitch = pi/2 takes getEulerFromQuaternion's gimbal branch, roll comes out 0
  {
    const double rpy[3] = {0.3, 0.5 * M_PI, 0.2};
    double t[10];
    pose_template(xyz, rpy, t);
    CHECK(t[7] == 0.0);
    CHECK(t[8] == 0.5 * M_PI);
    CHECK(std::fabs(t[3] * t[3] + t[4] * t[4] + t[5] * t[5] + t[6] * t[6] - 1.0) < 1e-15);
  }

  // trunc_step_counter: the smallest sc with sc / freq > len, by brute force
  {
    const double len[4] = {8.0, 0.0, 0.1, 1.0 / 3.0};
    const int freq[4] = {240, 240, 30, 48};
    for (int i = 0; i < 4; ++i) {
      int sc = 0;
      while (!((double)sc / freq[i] > len[i])) ++sc;
      CHECK(trunc_step_counter(len[i], freq[i]) == sc);
    }
    CHECK(trunc_step_counter(8.0, 240) == 1921 && trunc_step_counter(0.0, 240) == 1);
  }

  // check_env_rows: a NaN ixx in row 2 is refused under the caller's name
  {
    gpd_drone_params P;
    CHECK(default_params(GPD_MODEL_CF2X, &P) == GPD_OK);
    std::vector<gpd_env_params> rows(4, env_row_of(P));
    CHECK(check_env_rows("gpd_create_het", rows.data(), (int)rows.size()) == GPD_OK);
    rows[2].ixx = std::numeric_limits<double>::quiet_NaN();
    CHECK(check_env_rows("gpd_create_het", rows.data(), (int)rows.size()) == GPD_EINVAL);
    CHECK(g_err == "gpd_create_het: env_params field ixx of env 2 must be finite and > 0");
  }

  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
