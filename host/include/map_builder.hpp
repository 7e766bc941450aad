// map_builder.hpp -- the host side of fid_build_map_cam (include/fid_abi.h: "building the map"): collect the markers of the frames of
// a recording, build the map of the fiducials they show by bundle adjustment on the device, and hand it on as the entries fid_set_map
// takes or as the file fiducial_slam reads as its map_file.  Header only; needs nothing but the C-ABI.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "fid_abi.h"

namespace fiducials_amd {

class MapBuilder {
public:
    // ctx: any aruco context (its map, if it has one, is neither used nor changed); it is borrowed, not owned
    explicit MapBuilder(fid_ctx *ctx) : ctx_(ctx) {}

    // the markers of one frame (fid_detect's output); a frame without markers may be added, it is reported as FID_BUILD_VIEW_FEW
    void addView(const fid_marker *markers, int n) { views_.emplace_back(markers, markers + (n > 0 ? n : 0)); }
    size_t size() const { return views_.size(); }
    void clear() { views_.clear(); }

    // fid_build_map_cam over the views added so far.  fixed: the entries that define the map frame.  markers: every id seen;
    // entries (may be NULL): the FIXED and SOLVED ones as fid_set_map takes them; views (may be NULL): one record per added view.
    fid_status build(const fid_camera &cam, const std::vector<fid_map_entry> &fixed, const fid_build_opts &opts, fid_build_out *out,
                     std::vector<fid_build_marker> *markers, std::vector<fid_map_entry> *entries = nullptr, std::vector<fid_build_view> *views = nullptr) const
    {
        size_t cap = 1, total = 0;
        for (const auto &v : views_) {
            cap = v.size() > cap ? v.size() : cap;
            total += v.size();
        }
        std::vector<fid_marker> packed(views_.size() * cap);
        std::vector<int32_t> n(views_.size());
        for (size_t i = 0; i < views_.size(); i++) {
            n[i] = (int32_t)views_[i].size();
            for (size_t k = 0; k < views_[i].size(); k++) packed[i * cap + k] = views_[i][k];
        }
        std::vector<fid_build_marker> mout(total > 0 ? total : 1);  // (no more ids than markers)
        std::vector<fid_build_view> vout(views_.size());
        int32_t n_markers = 0;
        const fid_status rc = fid_build_map_cam(ctx_, &cam, packed.data(), n.data(), (int32_t)views_.size(), (int32_t)cap, fixed.data(), (int32_t)fixed.size(),
                                                &opts, out, mout.data(), (int32_t)mout.size(), &n_markers, vout.empty() ? nullptr : vout.data());
        if (rc != FID_OK) return rc;
        mout.resize((size_t)n_markers);
        if (entries) {
            entries->clear();
            for (const fid_build_marker &m : mout)
                if (m.status == FID_BUILD_MARKER_FIXED || m.status == FID_BUILD_MARKER_SOLVED) entries->push_back(m.entry);
        }
        if (markers) *markers = mout;
        if (views) *views = vout;
        return rc;
    }

    // what buildRobust reports beside build's records: per added view v and list position p, obs_state[v][p] (FID_BUILD_OBS_*) and
    // obs_err_px[v][p]; the outlier observations per entry of `markers` and per view
    struct RobustReport {
        fid_build_robust_out out;
        std::vector<std::vector<uint8_t>> obs_state;
        std::vector<std::vector<double>> obs_err_px;
        std::vector<int32_t> marker_outliers, view_outliers;
    };

    // fid_build_map_robust_cam over the views added so far: build() for views that hold wrong detections (a wrong id, a moved
    // fiducial, a false positive, a blurred view); ropts.inlier_px has no default (FID_BUILD_ROBUST_RECOMMENDED_PX).
    fid_status buildRobust(const fid_camera &cam, const std::vector<fid_map_entry> &fixed, const fid_build_opts &opts, const fid_build_robust_opts &ropts,
                           fid_build_out *out, RobustReport *report, std::vector<fid_build_marker> *markers, std::vector<fid_map_entry> *entries = nullptr,
                           std::vector<fid_build_view> *views = nullptr) const
    {
        if (!report) return FID_E_INVALID_ARG;
        size_t cap = 1, total = 0;
        for (const auto &v : views_) {
            cap = v.size() > cap ? v.size() : cap;
            total += v.size();
        }
        std::vector<fid_marker> packed(views_.size() * cap);
        std::vector<int32_t> n(views_.size());
        for (size_t i = 0; i < views_.size(); i++) {
            n[i] = (int32_t)views_[i].size();
            for (size_t k = 0; k < views_[i].size(); k++) packed[i * cap + k] = views_[i][k];
        }
        std::vector<fid_build_marker> mout(total > 0 ? total : 1);
        std::vector<fid_build_view> vout(views_.size());
        std::vector<uint8_t> state(views_.size() * cap);
        std::vector<double> err(views_.size() * cap);
        std::vector<int32_t> mo(mout.size()), vo(views_.size());
        int32_t n_markers = 0;
        const fid_status rc = fid_build_map_robust_cam(ctx_, &cam, packed.data(), n.data(), (int32_t)views_.size(), (int32_t)cap, fixed.data(), (int32_t)fixed.size(),
                                                       &opts, &ropts, out, &report->out, mout.data(), (int32_t)mout.size(), &n_markers,
                                                       vout.empty() ? nullptr : vout.data(), state.data(), err.data(), mo.data(), vo.empty() ? nullptr : vo.data());
        if (rc != FID_OK) return rc;
        mout.resize((size_t)n_markers);
        mo.resize((size_t)n_markers);
        report->obs_state.assign(views_.size(), {});
        report->obs_err_px.assign(views_.size(), {});
        for (size_t i = 0; i < views_.size(); i++) {
            report->obs_state[i].assign(state.begin() + (long)(i * cap), state.begin() + (long)(i * cap + views_[i].size()));
            report->obs_err_px[i].assign(err.begin() + (long)(i * cap), err.begin() + (long)(i * cap + views_[i].size()));
        }
        report->marker_outliers = mo;
        report->view_outliers = vo;
        if (entries) {
            entries->clear();
            for (const fid_build_marker &m : mout)
                if (m.status == FID_BUILD_MARKER_FIXED || m.status == FID_BUILD_MARKER_SOLVED) entries->push_back(m.entry);
        }
        if (markers) *markers = mout;
        if (views) *views = vout;
        return rc;
    }

    // fiducial_slam's map file (fid_map_save_file) of a build's markers
    static fid_status save(const std::string &path, const std::vector<fid_build_marker> &markers)
    {
        return fid_map_save_file(path.c_str(), markers.empty() ? nullptr : markers.data(), (int32_t)markers.size());
    }

private:
    fid_ctx *ctx_;
    std::vector<std::vector<fid_marker>> views_;
};

}  // namespace fiducials_amd
