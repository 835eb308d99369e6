// Dense hand-off, the scene (include/sfmcore.h, "Dense hand-off"): what
// openMVG2openMVS / DenseBuilder::save() collect, from the arrays that
// sfm_reconstruct returns.  Host only: integer work over the tracks, and one
// rotation per registered image.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "recon.h"
#include "rot_aa.h"

using namespace sfm;

struct sfm_dense_scene {
    std::vector<double> K, R, C;
    std::vector<int32_t> platform_wh, image_src, image_platform, image_pose;
    std::vector<float> vert_X;
    std::vector<int64_t> vert_off, vert_pt;
    std::vector<uint32_t> vert_view;
    int64_t n_short = 0;
};

namespace {

void build(const char* who, const sfm_ba_problem* P, const double* intr, const double* extr, const double* X,
           const int32_t* wh, const uint8_t* registered, const uint8_t* pt_ok, const uint8_t* keep_obs,
           sfm_dense_scene& sc) {
    recon_check_tracks(who, P);
    const int32_t cm = P->camera_model;
    SFM_REQUIRE(cm == SFM_CAM_PINHOLE || cm == SFM_CAM_SNAVELY || cm == SFM_CAM_RADIAL3, SFM_ERR_INVALID_ARG,
                "%s: unknown camera_model %d", who, cm);
    SFM_REQUIRE(cm != SFM_CAM_SNAVELY, SFM_ERR_UNSUPPORTED, "%s: SFM_CAM_SNAVELY has no principal point, so no K", who);
    const int iw = cm == SFM_CAM_RADIAL3 ? 6 : 4;
    SFM_REQUIRE(P->n_intr >= 0 && (P->n_intr == 0 || intr) && (P->n_img == 0 || (P->img_intr && extr && wh)) &&
                    (P->n_pt == 0 || X),
                SFM_ERR_INVALID_ARG, "%s: null argument", who);
    // platforms: one per block, in block order
    sc.K.assign(9 * (size_t)P->n_intr, 0.0);
    sc.platform_wh.assign(2 * (size_t)P->n_intr, 0);
    for (int32_t b = 0; b < P->n_intr; ++b) {
        const double* k = intr + (size_t)iw * b;
        for (int a = 0; a < iw; ++a)
            SFM_REQUIRE(std::isfinite(k[a]), SFM_ERR_INVALID_ARG, "%s: intrinsics block %d is not finite", who, b);
        double* K = &sc.K[9 * (size_t)b];
        K[0] = k[0];
        K[4] = cm == SFM_CAM_RADIAL3 ? k[0] : k[1];
        K[2] = cm == SFM_CAM_RADIAL3 ? k[1] : k[2];
        K[5] = cm == SFM_CAM_RADIAL3 ? k[2] : k[3];
        K[8] = 1.0;
    }
    std::vector<uint8_t> seen((size_t)P->n_intr, 0);
    for (int32_t i = 0; i < P->n_img; ++i) {
        const int32_t b = P->img_intr[i], w = wh[2 * i], h = wh[2 * i + 1];
        SFM_REQUIRE(b >= 0 && b < P->n_intr, SFM_ERR_INVALID_ARG, "%s: image %d names intrinsics block %d of %d", who, i,
                    b, P->n_intr);
        SFM_REQUIRE(w > 0 && h > 0, SFM_ERR_INVALID_ARG, "%s: image %d has a non-positive size", who, i);
        int32_t* pw = &sc.platform_wh[2 * (size_t)b];
        if (!seen[b]) {
            seen[b] = 1;
            pw[0] = w;
            pw[1] = h;
        }
        SFM_REQUIRE(pw[0] == w && pw[1] == h, SFM_ERR_INVALID_ARG,
                    "%s: image %d is %d x %d, intrinsics block %d has %d x %d images", who, i, w, h, b, pw[0], pw[1]);
    }
    // images: the registered ones, ascending
    std::vector<int32_t> scene_id((size_t)P->n_img, -1), n_poses((size_t)P->n_intr, 0);
    for (int32_t i = 0; i < P->n_img; ++i) {
        if (registered && !registered[i]) continue;
        const double* e = extr + 6 * (size_t)i;
        for (int a = 0; a < 6; ++a)
            SFM_REQUIRE(std::isfinite(e[a]), SFM_ERR_INVALID_ARG, "%s: the pose of image %d is not finite", who, i);
        scene_id[i] = (int32_t)sc.image_src.size();
        sc.image_src.push_back(i);
        sc.image_platform.push_back(P->img_intr[i]);
        sc.image_pose.push_back(n_poses[P->img_intr[i]]++);
        double R[9];
        aa_to_matrix(e, R);
        sc.R.insert(sc.R.end(), R, R + 9);
        for (int a = 0; a < 3; ++a) sc.C.push_back(-(R[a] * e[3] + R[3 + a] * e[4] + R[6 + a] * e[5]));
    }
    // vertices: the distinct registered views of each kept point, ascending
    sc.vert_off.assign(1, 0);
    std::vector<int64_t> stamp(sc.image_src.size(), -1);   // the last point that listed the view
    std::vector<uint32_t> views;
    for (int64_t p = 0; p < P->n_pt; ++p) {
        if (pt_ok && !pt_ok[p]) continue;
        views.clear();
        for (int64_t o = P->pt_offsets[p]; o < P->pt_offsets[p + 1]; ++o) {
            if (keep_obs && !keep_obs[o]) continue;
            const int32_t id = scene_id[P->obs_img[o]];
            if (id < 0 || stamp[id] == p) continue;
            stamp[id] = p;
            views.push_back((uint32_t)id);
        }
        if (views.size() < 2) {
            ++sc.n_short;
            continue;
        }
        std::sort(views.begin(), views.end());
        for (int a = 0; a < 3; ++a) {
            SFM_REQUIRE(std::isfinite(X[3 * p + a]), SFM_ERR_INVALID_ARG, "%s: point %lld is not finite", who,
                        (long long)p);
            sc.vert_X.push_back((float)X[3 * p + a]);
        }
        sc.vert_view.insert(sc.vert_view.end(), views.begin(), views.end());
        sc.vert_off.push_back((int64_t)sc.vert_view.size());
        sc.vert_pt.push_back(p);
    }
}

template <class T>
void copy_out(const std::vector<T>& v, T* dst) {
    if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(T));
}

}  // namespace

extern "C" int sfm_dense_scene_build(const sfm_ba_problem* tracks, const double* intr, const double* extr,
                                     const double* X, const int32_t* wh, const uint8_t* registered,
                                     const uint8_t* pt_ok, const uint8_t* keep_obs, sfm_dense_scene** scene) {
    return guarded([&] {
        SFM_REQUIRE(scene, SFM_ERR_INVALID_ARG, "sfm_dense_scene_build: null scene");
        *scene = nullptr;
        sfm_dense_scene* sc = new sfm_dense_scene;
        try {
            build("sfm_dense_scene_build", tracks, intr, extr, X, wh, registered, pt_ok, keep_obs, *sc);
        } catch (...) {
            delete sc;
            throw;
        }
        *scene = sc;
        return SFM_OK;
    });
}

extern "C" int sfm_dense_scene_get_info(const sfm_dense_scene* scene, sfm_dense_scene_info* info) {
    return guarded([&] {
        SFM_REQUIRE(scene && info, SFM_ERR_INVALID_ARG, "sfm_dense_scene_get_info: null argument");
        info->n_platforms = (int32_t)scene->platform_wh.size() / 2;
        info->n_images = (int32_t)scene->image_src.size();
        info->n_vertices = (int64_t)scene->vert_pt.size();
        info->n_views = (int64_t)scene->vert_view.size();
        info->n_short = scene->n_short;
        return SFM_OK;
    });
}

extern "C" int sfm_dense_scene_fetch(const sfm_dense_scene* scene, double* K, int32_t* platform_wh, int32_t* image_src,
                                     int32_t* image_platform, int32_t* image_pose, double* R, double* C, float* vert_X,
                                     int64_t* vert_off, uint32_t* vert_view, int64_t* vert_pt) {
    return guarded([&] {
        SFM_REQUIRE(scene, SFM_ERR_INVALID_ARG, "sfm_dense_scene_fetch: null scene");
        copy_out(scene->K, K);
        copy_out(scene->platform_wh, platform_wh);
        copy_out(scene->image_src, image_src);
        copy_out(scene->image_platform, image_platform);
        copy_out(scene->image_pose, image_pose);
        copy_out(scene->R, R);
        copy_out(scene->C, C);
        copy_out(scene->vert_X, vert_X);
        copy_out(scene->vert_off, vert_off);
        copy_out(scene->vert_view, vert_view);
        copy_out(scene->vert_pt, vert_pt);
        return SFM_OK;
    });
}

extern "C" int sfm_dense_scene_destroy(sfm_dense_scene* scene) {
    delete scene;
    return SFM_OK;
}
