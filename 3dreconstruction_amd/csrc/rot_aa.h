// A rotation matrix as its angle-axis vector, on the host: what camera
// resection (resect.cpp) and relative pose (relpose.cpp) report their
// rotations as; and the way back, for the dense scene's poses (dense_scene.cpp).
#pragma once
#include <cmath>

namespace sfm {
namespace {

// rot::matrix_to_aa (include/sfm/world.hpp): a rotation matrix as its angle-axis vector
inline void matrix_to_aa(const double* R, double* w) {
    const double tr = R[0] + R[4] + R[8];
    double q[4];
    if (tr >= 0) {
        double t = std::sqrt(tr + 1.0);
        q[0] = 0.5 * t; t = 0.5 / t;
        q[1] = (R[7] - R[5]) * t; q[2] = (R[2] - R[6]) * t; q[3] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = std::sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
        q[i + 1] = 0.5 * t; t = 0.5 / t;
        q[0] = (R[k * 3 + j] - R[j * 3 + k]) * t;
        q[j + 1] = (R[j * 3 + i] + R[i * 3 + j]) * t;
        q[k + 1] = (R[k * 3 + i] + R[i * 3 + k]) * t;
    }
    if (q[0] < 0) for (double& v : q) v = -v;
    const double sn = std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (sn < 1e-300) { w[0] = 2 * q[1]; w[1] = 2 * q[2]; w[2] = 2 * q[3]; return; }
    const double th = 2.0 * std::atan2(sn, q[0]);
    for (int a = 0; a < 3; ++a) w[a] = q[a + 1] * th / sn;
}

// rot::aa_to_matrix (include/sfm/world.hpp): R(w), row-major, by Rodrigues' formula
inline void aa_to_matrix(const double* w, double* R) {
    const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (th < 1e-300) {
        for (int a = 0; a < 9; ++a) R[a] = (a % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double u[3] = {w[0] / th, w[1] / th, w[2] / th}, c = std::cos(th), s = std::sin(th), oc = 1 - c;
    R[0] = c + oc * u[0] * u[0];        R[1] = oc * u[0] * u[1] - s * u[2]; R[2] = oc * u[0] * u[2] + s * u[1];
    R[3] = oc * u[1] * u[0] + s * u[2]; R[4] = c + oc * u[1] * u[1];        R[5] = oc * u[1] * u[2] - s * u[0];
    R[6] = oc * u[2] * u[0] - s * u[1]; R[7] = oc * u[2] * u[1] + s * u[0]; R[8] = c + oc * u[2] * u[2];
}

}  // namespace
}  // namespace sfm
