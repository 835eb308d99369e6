// ColorizeTracks: OpenMVG's greedy track colouring (what sparseBuilder::colorize()
// runs, sparseBuilder.cpp:1601-1630) over a WorldStructure whose points carry
// their tracks (observed_frames_), over a backend policy
//   int colorize(const sfm_ba_problem& tracks, const int32_t* wh, const uint8_t* pt_ok, const uint8_t* keep_obs,
//                const int32_t* channels, const int64_t* img_off, const uint8_t* pixels, uint8_t* rgb,
//                int32_t* view, sfm_colorize_stats* stats) const;   // SFM_OK / SFM_ERR_*
//   const char* last_error() const;
// sfm.hpp binds it to the GPU (sfm_colorize: the device chooses the view of
// every point, the host samples); HostColorizeBackend is the host twin
// (sfm_colorize_host), with the same bytes.  Header-only.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <vector>

#include "../../../include/sfmcore.h"
#include "world.hpp"

namespace sfm {

// One image's pixels: row-major, interleaved, row stride w * channels,
// channels 1 or 3.  data == nullptr: not loaded (an image that no point to
// colour is seen in may stay so).
struct ColorImage {
    const uint8_t* data;
    int32_t w, h, channels;
};

// The pixel pool of the C-ABI over images the caller holds one by one: byte
// offsets from the lowest address among them, nothing is copied.
struct ColorPool {
    std::vector<int32_t> wh, channels;
    std::vector<int64_t> img_off;
    const uint8_t* pixels = nullptr;
    explicit ColorPool(const std::vector<ColorImage>& images) {
        uintptr_t base = UINTPTR_MAX;
        for (const auto& im : images)
            if (im.data) base = std::min(base, reinterpret_cast<uintptr_t>(im.data));
        for (const auto& im : images) {
            wh.push_back(im.w);
            wh.push_back(im.h);
            channels.push_back(im.channels);
            img_off.push_back(im.data ? (int64_t)(reinterpret_cast<uintptr_t>(im.data) - base) : -1);
        }
        if (base != UINTPTR_MAX) pixels = reinterpret_cast<const uint8_t*>(base);
        wh.resize(wh.size() + 2, 1);   // (never empty)
        channels.push_back(1);
        img_off.push_back(-1);
    }
};

struct HostColorizeBackend {
    int colorize(const sfm_ba_problem& tracks, const int32_t* wh, const uint8_t* pt_ok, const uint8_t* keep_obs,
                 const int32_t* channels, const int64_t* img_off, const uint8_t* pixels, uint8_t* rgb, int32_t* view,
                 sfm_colorize_stats* stats) const {
        return sfm_colorize_host(&tracks, wh, pt_ok, keep_obs, channels, img_off, pixels, rgb, view, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};

// colors[p] = the colour of world point p (index order), 0 0 0 where it has no
// observation in `images`; images[k] and pixels[k] belong together.  pt_ok
// (optional, per world point): the points to colour.  False when the call
// failed (nothing is written then).
template <class Backend>
bool ColorizeTracks(const Backend& backend, const WorldStructure& world, const std::vector<Image::Ptr>& images,
                    const std::vector<ColorImage>& pixels, std::vector<std::array<uint8_t, 3>>& colors,
                    const std::vector<uint8_t>* pt_ok = nullptr, sfm_colorize_stats* stats = nullptr) {
    if (pixels.size() != images.size() || (pt_ok && pt_ok->size() != world.pointsByIdx().size())) {
        std::fprintf(stderr, "ColorizeTracks failed: %zu images, %zu pixel arrays\n", images.size(), pixels.size());
        return false;
    }
    std::unordered_map<const Image*, int32_t> slot;
    for (size_t k = 0; k < images.size(); ++k) slot[images[k].get()] = (int32_t)k;
    const auto& pts = world.pointsByIdx();
    std::vector<int64_t> off(1, 0);
    std::vector<int32_t> obs_img;
    std::vector<double> obs_uv;
    for (const auto& p : pts) {
        for (const auto& ob : p->observed_frames_) {
            const auto it = slot.find(ob.first.get());
            if (it == slot.end()) continue;
            obs_img.push_back(it->second);
            obs_uv.push_back(ob.second.x);
            obs_uv.push_back(ob.second.y);
        }
        off.push_back((int64_t)obs_img.size());
    }
    sfm_ba_problem P{};
    P.n_img = (int32_t)images.size();
    P.n_pt = (int64_t)pts.size();
    P.n_obs = (int64_t)obs_img.size();
    obs_img.push_back(0);   // (never empty)
    obs_uv.resize(obs_uv.size() + 2, 0.0);
    P.pt_offsets = off.data();
    P.obs_img = obs_img.data();
    P.obs_uv = obs_uv.data();
    const ColorPool pool(pixels);
    std::vector<uint8_t> rgb(3 * pts.size() + 3);
    const int rc = backend.colorize(P, pool.wh.data(), pt_ok ? pt_ok->data() : nullptr, nullptr, pool.channels.data(),
                                    pool.img_off.data(), pool.pixels, rgb.data(), nullptr, stats);
    if (rc != SFM_OK) {
        std::fprintf(stderr, "ColorizeTracks failed: %s (code %d)\n", backend.last_error(), rc);
        return false;
    }
    colors.resize(pts.size());
    for (size_t p = 0; p < pts.size(); ++p) colors[p] = {rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
    return true;
}

}  // namespace sfm
