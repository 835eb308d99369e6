// SIFT_Image_describer: the reference's feature extractor
// (src/nonFree/sift/SIFT_describer.hpp: Params, Set_configuration_preset,
// Describe) and sparseBuilder::detectFeature() over a backend policy
//   int sift(const uint8_t* gray, int32_t n_img, int32_t w, int32_t h, const sfm_sift_options&,
//            int64_t cap_per_img, float* xyso, uint8_t* desc, int64_t* n_feat, sfm_sift_summary*);
//   const char* last_error() const;
// sfm.hpp binds it to the GPU (sfm_sift); HostSiftBackend is the serial host
// twin (sfm_sift_host).  Images are 8-bit gray buffers: decoding image files
// stays with the caller.  Limits: first_octave -1 (the ULTRA preset) and
// masks are not supported (lastError() == SFM_ERR_UNSUPPORTED).
// Header-only.
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/sfmcore.h"

namespace sfm {

enum EDESCRIBER_PRESET { NORMAL_PRESET = 0, HIGH_PRESET, ULTRA_PRESET };

// SIFT_Regions: SIOPointFeature (x, y, scale, orientation) and 128 bytes each
struct SiftRegions {
    std::vector<std::array<float, 4>> features;
    std::vector<std::array<uint8_t, 128>> descriptors;
    size_t RegionCount() const { return features.size(); }
};

// an 8-bit gray image held by the caller (row-major, w * h bytes)
struct GrayImage {
    const uint8_t* data;
    int32_t w, h;
};

struct HostSiftBackend {
    int sift(const uint8_t* gray, int32_t n_img, int32_t w, int32_t h, const sfm_sift_options& o, int64_t cap,
             float* xyso, uint8_t* desc, int64_t* n_feat, sfm_sift_summary* sm) const {
        return sfm_sift_host(gray, n_img, w, h, &o, cap, xyso, desc, n_feat, sm);
    }
    const char* last_error() const { return sfm_last_error(); }
};

template <class Backend>
class BasicSiftDescriber {
   public:
    struct Params {
        Params(int first_octave = 0, int num_octaves = 6, int num_scales = 3, float edge_threshold = 10.0f,
               float peak_threshold = 0.04f, bool root_sift = true)
            : _first_octave(first_octave), _num_octaves(num_octaves), _num_scales(num_scales),
              _edge_threshold(edge_threshold), _peak_threshold(peak_threshold), _root_sift(root_sift) {}
        int _first_octave, _num_octaves, _num_scales;
        float _edge_threshold, _peak_threshold;
        bool _root_sift;
    };

    explicit BasicSiftDescriber(Backend backend, const Params& params = Params(), bool bOrientation = true)
        : backend_(std::move(backend)), _params(params), _bOrientation(bOrientation) {}

    bool Set_configuration_preset(EDESCRIBER_PRESET preset) {
        switch (preset) {
            case NORMAL_PRESET: _params._peak_threshold = 0.04f; break;
            case HIGH_PRESET: _params._peak_threshold = 0.01f; break;
            case ULTRA_PRESET: _params._peak_threshold = 0.01f; _params._first_octave = -1; break;
            default: return false;
        }
        return true;
    }
    Params& params() { return _params; }
    int lastError() const { return last_rc_; }
    const sfm_sift_summary& summary() const { return summary_; }

    // one image
    SiftRegions Describe(const uint8_t* gray, int32_t w, int32_t h) {
        std::vector<SiftRegions> r = Describe(std::vector<GrayImage>{GrayImage{gray, w, h}});
        return r.empty() ? SiftRegions{} : std::move(r[0]);
    }

    // many images, of any sizes: those of one size go through one call.  On
    // failure lastError() is set and the regions come back empty.
    std::vector<SiftRegions> Describe(const std::vector<GrayImage>& images) {
        std::vector<SiftRegions> out(images.size());
        last_rc_ = SFM_OK;
        summary_ = sfm_sift_summary{};
        std::map<std::pair<int32_t, int32_t>, std::vector<size_t>> by_size;
        for (size_t i = 0; i < images.size(); ++i) by_size[{images[i].w, images[i].h}].push_back(i);
        sfm_sift_options o{};
        o.n_octaves = _params._num_octaves; o.n_scales = _params._num_scales; o.first_octave = _params._first_octave;
        o.edge_threshold = _params._edge_threshold; o.peak_threshold = _params._peak_threshold;
        o.root_sift = _params._root_sift ? 1 : 0; o.orientation = _bOrientation ? 1 : 0;
        for (const auto& g : by_size) {
            const int32_t w = g.first.first, h = g.first.second, n = (int32_t)g.second.size();
            const size_t wh = (size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0);
            std::vector<uint8_t> gray(wh * n + 1);
            for (int32_t i = 0; i < n; ++i)
                std::copy(images[g.second[i]].data, images[g.second[i]].data + wh, gray.begin() + wh * i);
            std::vector<int64_t> n_feat(n, 0);
            // room for 4096 features per image; once more at the largest count if an image has more
            sfm_sift_summary sm{};
            int64_t cap = 4096;
            std::vector<float> xyso((size_t)cap * n * 4);
            std::vector<uint8_t> desc((size_t)cap * n * 128);
            int rc = backend_.sift(gray.data(), n, w, h, o, cap, xyso.data(), desc.data(), n_feat.data(), &sm);
            if (rc == SFM_OK && sm.n_overflow > 0) {
                for (int64_t v : n_feat) cap = v > cap ? v : cap;
                xyso.resize((size_t)cap * n * 4);
                desc.resize((size_t)cap * n * 128);
                rc = backend_.sift(gray.data(), n, w, h, o, cap, xyso.data(), desc.data(), n_feat.data(), &sm);
            }
            if (rc != SFM_OK) {
                last_rc_ = rc;
                std::fprintf(stderr, "SIFT extraction failed: %s (code %d)\n", backend_.last_error(), rc);
                return std::vector<SiftRegions>(images.size());
            }
            summary_.n_images += sm.n_images; summary_.n_keypoints += sm.n_keypoints;
            summary_.n_features += sm.n_features; summary_.n_written += sm.n_written;
            summary_.kernel_ms = sm.kernel_ms;
            for (int32_t i = 0; i < n; ++i) {
                SiftRegions& r = out[g.second[i]];
                r.features.resize((size_t)n_feat[i]);
                r.descriptors.resize((size_t)n_feat[i]);
                for (int64_t k = 0; k < n_feat[i]; ++k) {
                    const size_t row = (size_t)i * cap + k;
                    std::copy(&xyso[4 * row], &xyso[4 * row] + 4, r.features[k].begin());
                    std::copy(&desc[128 * row], &desc[128 * row] + 128, r.descriptors[k].begin());
                }
            }
        }
        return out;
    }

   private:
    Backend backend_;
    Params _params;
    bool _bOrientation;
    sfm_sift_summary summary_{};
    int last_rc_ = SFM_OK;
};

class HostSIFT_Image_describer : public BasicSiftDescriber<HostSiftBackend> {
   public:
    explicit HostSIFT_Image_describer(const Params& params = Params(), bool bOrientation = true)
        : BasicSiftDescriber<HostSiftBackend>(HostSiftBackend{}, params, bOrientation) {}
};

// sparseBuilder::detectFeature() on in-memory images: <dir>/<stem>.feat and
// <dir>/<stem>.desc per image and <dir>/image_describer.json, in the layouts
// the file-staged match() reads.  false on failure (sfm_last_error() says why).
template <class Describer>
bool detectFeature(Describer& describer, const std::vector<GrayImage>& images, const std::vector<std::string>& stems,
                   const std::string& dir) {
    if (images.size() != stems.size()) return false;
    const std::vector<SiftRegions> regions = describer.Describe(images);
    if (describer.lastError() != SFM_OK) return false;
    for (size_t i = 0; i < images.size(); ++i) {
        const SiftRegions& r = regions[i];
        const std::string stem = dir + "/" + stems[i];
        const float* f = r.features.empty() ? nullptr : r.features[0].data();
        const uint8_t* d = r.descriptors.empty() ? nullptr : r.descriptors[0].data();
        if (sfm_mvg_write_feat((stem + ".feat").c_str(), f, (int64_t)r.features.size()) != SFM_OK) return false;
        if (sfm_mvg_write_desc((stem + ".desc").c_str(), d, (int64_t)r.descriptors.size()) != SFM_OK) return false;
    }
    const std::string path = dir + "/image_describer.json";
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    const auto& p = describer.params();
    std::fprintf(f,
                 "{\n  \"regions_type\": {\n    \"polymorphic_id\": 2147483649,\n"
                 "    \"polymorphic_name\": \"SIFT_Regions\",\n    \"ptr_wrapper\": {\"valid\": 1, \"data\": {}}\n  },\n"
                 "  \"image_describer\": {\n    \"polymorphic_id\": 2147483649,\n"
                 "    \"polymorphic_name\": \"SIFT_Image_describer\",\n    \"ptr_wrapper\": {\"valid\": 1, \"data\": {\n"
                 "      \"params\": {\"first_octave\": %d, \"num_octaves\": %d, \"num_scales\": %d,\n"
                 "                 \"edge_threshold\": %.9g, \"peak_threshold\": %.9g, \"root_sift\": %s},\n"
                 "      \"bOrientation\": true}}\n  }\n}\n",
                 p._first_octave, p._num_octaves, p._num_scales, (double)p._edge_threshold, (double)p._peak_threshold,
                 p._root_sift ? "true" : "false");
    return std::fclose(f) == 0;
}

}  // namespace sfm
