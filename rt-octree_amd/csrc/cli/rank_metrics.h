// rank_metrics.h -- the RANK_METRICS line of `volrend_headless --gpus N`: a child (--rank_report) prints the SUMS of its
// frames' PSNR, SSIM and SMAPE and the frame count next to its RANK_REPORT line; the parent adds the ranks' sums up and
// divides once, so the printed means are the means over all frames whatever N is.  One formatter and one parser, shared by
// both sides (and called on hand-made lines by tools/sanitize/png_fuzz.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

namespace rto {

struct MetricSums {
    double psnr = 0.0, ssim = 0.0, smape = 0.0;
    long frames = 0;
    void add(double p, double s, double m) { psnr += p, ssim += s, smape += m, ++frames; }
    void merge(const MetricSums& o) { psnr += o.psnr, ssim += o.ssim, smape += o.smape, frames += o.frames; }
};

// %.17g round-trips a double; inf and nan print and parse as such
inline std::string format_rank_metrics(const MetricSums& s) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), "RANK_METRICS %.17g %.17g %.17g %ld", s.psnr, s.ssim, s.smape, s.frames);
    return buf;
}

// false: not such a line (the parent relays it like any other output)
inline bool parse_rank_metrics(const std::string& line, MetricSums* s) {
    MetricSums t;
    char tail = 0;
    if (std::sscanf(line.c_str(), "RANK_METRICS %lf %lf %lf %ld %c", &t.psnr, &t.ssim, &t.smape, &t.frames, &tail) != 4 || t.frames < 0)
        return false;
    *s = t;
    return true;
}

// the three report lines after the timing lines: the mean over frames of the per-frame value (denoiser/metrics.py:50-58)
inline std::string format_metric_means(const MetricSums& s) {
    char buf[256];
    const double n = s.frames > 0 ? (double)s.frames : 1.0;
    std::snprintf(buf, sizeof(buf), "psnr:   %.10f\nssim:   %.10f\nsmape:  %.10f\n", s.psnr / n, s.ssim / n, s.smape / n);
    return buf;
}

// one pose's values.  A child prints one RANK_FRAME_METRICS line per pose it rendered; the parent collects them and writes the
// one metrics.json of the run, so that the file does not depend on N
struct FrameRow {
    long pose = 0;
    std::string name;
    double mse = 0.0, psnr = 0.0, smape = 0.0, ssim = 0.0;
};

inline std::string format_frame_metrics(const FrameRow& r) {
    char buf[512];
    std::snprintf(buf, sizeof(buf), "RANK_FRAME_METRICS %ld %.17g %.17g %.17g %.17g %s", r.pose, r.mse, r.psnr, r.smape, r.ssim, r.name.c_str());
    return buf;
}

inline bool parse_frame_metrics(const std::string& line, FrameRow* r) {
    FrameRow t;
    int used = 0;
    if (std::sscanf(line.c_str(), "RANK_FRAME_METRICS %ld %lf %lf %lf %lf %n", &t.pose, &t.mse, &t.psnr, &t.smape, &t.ssim, &used) != 5 || used <= 0 ||
        t.pose < 0)
        return false;
    t.name = line.substr((size_t)used);
    if (t.name.empty()) return false;
    *r = t;
    return true;
}

// a double as Python's json module reads it back bit for bit (NaN / Infinity / -Infinity for the non-finite ones)
inline std::string json_double(double v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "Infinity" : "-Infinity";
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%.17g", v);
    return buf;
}

// metrics.json: {"frames": [{"pose", "name", "mse", "psnr", "smape", "ssim"} ... in pose order], "mean": {"psnr", "ssim", "smape"}, "count"}
inline bool write_metrics_json(const std::string& path, std::vector<FrameRow> rows) {
    std::sort(rows.begin(), rows.end(), [](const FrameRow& a, const FrameRow& b) { return a.pose < b.pose; });
    MetricSums sums;
    for (const FrameRow& r : rows) sums.add(r.psnr, r.ssim, r.smape);
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    std::fputs("{\n  \"frames\": [", f);
    for (size_t i = 0; i < rows.size(); ++i) {
        const FrameRow& r = rows[i];
        std::string name;
        for (char c : r.name) {
            if (c == '"' || c == '\\') name.push_back('\\');
            name.push_back((unsigned char)c < 0x20 ? '?' : c);
        }
        std::fprintf(f, "%s\n    {\"pose\": %ld, \"name\": \"%s\", \"mse\": %s, \"psnr\": %s, \"smape\": %s, \"ssim\": %s}", i ? "," : "", r.pose,
                     name.c_str(), json_double(r.mse).c_str(), json_double(r.psnr).c_str(), json_double(r.smape).c_str(), json_double(r.ssim).c_str());
    }
    const double n = sums.frames > 0 ? (double)sums.frames : 1.0;
    std::fprintf(f, "\n  ],\n  \"mean\": {\"psnr\": %s, \"ssim\": %s, \"smape\": %s},\n  \"count\": %ld\n}\n", json_double(sums.psnr / n).c_str(),
                 json_double(sums.ssim / n).c_str(), json_double(sums.smape / n).c_str(), sums.frames);
    return std::fclose(f) == 0;
}

}  // namespace rto
