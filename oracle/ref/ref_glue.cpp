// ref_glue.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Joins the reference's ORBextractor_old.cc (compiled from the generated copy under
// oracle/_ref/gen/) to the oracle's primitives and exports it through a C ABI (oracle/ref_py.py).
// The ORB-SLAM logic that runs behind these entry points is the reference's own object code; the
// OpenCV primitives and the pyramid loop are the oracle's (oracle/ref/README.md).
#include <algorithm>

#include "ORBextractor.h"
#include "orb_oracle.h"

// ---- OpenCV primitives on the oracle ---------------------------------------------------------
namespace cv {

void FAST(const Mat& image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmaxSuppression) {
    if (!nonmaxSuppression) ref_shim_abort("FAST: only nonmaxSuppression = true");
    keypoints.clear();
    if (image.empty()) return;
    std::vector<oracle_kp> buf((size_t)image.rows * image.cols + 1);
    int n = oracle_fast(image.data, (int)image.step, 0, 0, image.cols, image.rows, threshold, buf.data(),
                        (int)buf.size());
    keypoints.resize(n);
    for (int i = 0; i < n; ++i) {
        KeyPoint& k = keypoints[i];
        k.pt.x = buf[i].x, k.pt.y = buf[i].y, k.size = buf[i].size, k.angle = buf[i].angle;
        k.response = buf[i].response, k.octave = buf[i].octave, k.class_id = buf[i].class_id;
    }
}

void GaussianBlur(const Mat& src, Mat& dst, Size ksize, double sigmaX, double sigmaY, int borderType) {
    if (ksize.width != 7 || ksize.height != 7 || sigmaX != 2 || sigmaY != 2 || borderType != BORDER_REFLECT_101)
        ref_shim_abort("GaussianBlur: only 7x7, sigma 2, BORDER_REFLECT_101");
    Mat in = src.clone();  // tight pitch, and src may be dst
    dst.create(in.rows, in.cols, CV_8UC1);
    if (dst.step != (size_t)dst.cols) ref_shim_abort("GaussianBlur: dst must be continuous");
    oracle_gaussian_blur(in.data, in.cols, in.rows, dst.data);
}

float fastAtan2(float y, float x) { return oracle_fast_atan2(y, x); }

}  // namespace cv

// ---- Android / accelerator names -------------------------------------------------------------
int FrameAHB::s_HardwareBufferUses = 0;
void AHardwareBuffer_describe(const AHardwareBuffer*, AHardwareBuffer_Desc*) { cv::ref_shim_abort("AHardwareBuffer_describe reached"); }
int AHardwareBuffer_lock(AHardwareBuffer*, uint64_t, int32_t, const void*, void**) { cv::ref_shim_abort("AHardwareBuffer_lock reached"); }
int AHardwareBuffer_unlock(AHardwareBuffer*, int32_t*) { cv::ref_shim_abort("AHardwareBuffer_unlock reached"); }

LynxHardwareAccelerator& LynxHardwareAccelerator::GetInstance() {
    static LynxHardwareAccelerator instance;
    return instance;
}

void LynxHardwareAccelerator::ComputePyramid(const cv::Mat& image, int nlevels, const std::vector<float>& invScaleFactor,
                                             std::vector<cv::Mat>& pyramid) {
    pyramid.resize(nlevels);
    for (int level = 0; level < nlevels; ++level) {
        float scale = invScaleFactor[level];
        int w = cvRound((float)image.cols * scale), h = cvRound((float)image.rows * scale);
        if (level == 0) {
            pyramid[0] = image.clone();
        } else {
            const cv::Mat& s = pyramid[level - 1];
            cv::Mat d(h, w, CV_8UC1);
            oracle_resize(s.data, s.cols, s.rows, (int)s.step, d.data, w, h, (int)d.step);
            pyramid[level] = d;
        }
    }
}

void LynxHardwareAccelerator::ComputeKeyPointsOctTree(std::vector<std::vector<cv::KeyPoint>>&, std::vector<cv::Mat>&, int,
                                                      int, int, int, int, std::vector<int>&, std::vector<float>&,
                                                      std::vector<int>&) {
    cv::ref_shim_abort("LynxHardwareAccelerator::ComputeKeyPointsOctTree reached");
}

// ---- C entry points --------------------------------------------------------------------------
namespace {

// the protected members, reached the way a subclass would
struct RefExtractor : ORB_SLAM3::ORBextractor {
    using ORB_SLAM3::ORBextractor::ORBextractor;
    void octree_levels(std::vector<std::vector<cv::KeyPoint>>& all) { ComputeKeyPointsOctTree(all); }
    std::vector<cv::KeyPoint> distribute(const std::vector<cv::KeyPoint>& keys, int minX, int maxX, int minY, int maxY,
                                         int N) {
        return DistributeOctTree(keys, minX, maxX, minY, maxY, N, 0);
    }
    const std::vector<int>& features_per_level() const { return mnFeaturesPerLevel; }
    const std::vector<int>& u_max() const { return umax; }
    const std::vector<cv::Point>& bit_pattern() const { return pattern; }
    const std::vector<float>& inv_scale() const { return mvInvScaleFactor; }
};

oracle_kp to_c(const cv::KeyPoint& k) {
    oracle_kp o;
    o.x = k.pt.x, o.y = k.pt.y, o.size = k.size, o.angle = k.angle, o.response = k.response;
    o.octave = k.octave, o.class_id = k.class_id;
    return o;
}

cv::KeyPoint from_c(const oracle_kp& o) {
    cv::KeyPoint k;
    k.pt.x = o.x, k.pt.y = o.y, k.size = o.size, k.angle = o.angle, k.response = o.response;
    k.octave = o.octave, k.class_id = o.class_id;
    return k;
}

}  // namespace

extern "C" {

// ORBextractor::operator()(InputArray, InputArray, vector<KeyPoint>&, OutputArray, vector<int>&).
// Returns its return value (monoIndex, -1 on an empty image), or -2 when cap is too small.
int ref_extract(int nfeatures, float scale_factor, int nlevels, int ini_th, int min_th, const uint8_t* img, int w,
                int h, int stride, int lap0, int lap1, oracle_kp* kps, uint8_t* desc, int cap, int* n_out) {
    *n_out = 0;
    RefExtractor ex(nfeatures, scale_factor, nlevels, ini_th, min_th);
    cv::Mat image = (img && w > 0 && h > 0) ? cv::Mat(h, w, CV_8UC1, (void*)img, (size_t)stride) : cv::Mat();
    cv::Mat mask, descriptors;
    std::vector<cv::KeyPoint> keypoints;
    std::vector<int> lap = {lap0, lap1};
    int mono = ex(image, mask, keypoints, descriptors, lap);
    if (mono < 0) return mono;
    int n = (int)keypoints.size();
    if (n > cap) return -2;
    for (int i = 0; i < n; ++i) {
        kps[i] = to_c(keypoints[i]);
        memcpy(desc + 32 * (size_t)i, descriptors.ptr(i), 32);
    }
    *n_out = n;
    return mono;
}

// ComputeKeyPointsOctTree on a pyramid built as operator() builds it: per-level keypoints in level
// coordinates, octree order, with angle.  lvl_count[nlevels]; returns the total, -2 on overflow.
int ref_extract_levels(int nfeatures, float scale_factor, int nlevels, int ini_th, int min_th, const uint8_t* img,
                       int w, int h, int stride, oracle_kp* kps, int cap, int* lvl_count) {
    if (!img || w <= 0 || h <= 0) return -1;
    RefExtractor ex(nfeatures, scale_factor, nlevels, ini_th, min_th);
    cv::Mat image(h, w, CV_8UC1, (void*)img, (size_t)stride);
    LynxHardwareAccelerator::GetInstance().ComputePyramid(image, nlevels, ex.inv_scale(), ex.mvImagePyramid);
    std::vector<std::vector<cv::KeyPoint>> all;
    ex.octree_levels(all);
    int off = 0;
    for (int level = 0; level < nlevels; ++level) {
        lvl_count[level] = (int)all[level].size();
        for (const cv::KeyPoint& k : all[level]) {
            if (off >= cap) return -2;
            kps[off++] = to_c(k);
        }
    }
    return off;
}

// DistributeOctTree on a candidate list; returns the number of keys kept (out holds min(that, cap)).
int ref_distribute_octree(const oracle_kp* keys, int n, int minX, int maxX, int minY, int maxY, int N, oracle_kp* out,
                          int cap) {
    RefExtractor ex(1000, 1.2f, 8, 20, 7);
    std::vector<cv::KeyPoint> v(n);
    for (int i = 0; i < n; ++i) v[i] = from_c(keys[i]);
    std::vector<cv::KeyPoint> r = ex.distribute(v, minX, maxX, minY, maxY, N);
    int m = (int)r.size();
    for (int i = 0; i < m && i < cap; ++i) out[i] = to_c(r[i]);
    return m;
}

// The constructor's tables: the six getters, then the protected vectors.  scale / inv_scale /
// sigma2 / inv_sigma2 / features_per_level: [nlevels]; umax16: [16]; pattern: [512][2].
void ref_tables(int nfeatures, float scale_factor, int nlevels, int* levels, float* scale_factor_out, float* scale,
                float* inv_scale, float* sigma2, float* inv_sigma2, int* features_per_level, int* umax16,
                int* pattern) {
    RefExtractor ex(nfeatures, scale_factor, nlevels, 20, 7);
    *levels = ex.GetLevels();
    *scale_factor_out = ex.GetScaleFactor();
    std::vector<float> a = ex.GetScaleFactors(), b = ex.GetInverseScaleFactors(), c = ex.GetScaleSigmaSquares(),
                       d = ex.GetInverseScaleSigmaSquares();
    if ((int)a.size() != nlevels || (int)b.size() != nlevels || (int)c.size() != nlevels ||
        (int)d.size() != nlevels || (int)ex.features_per_level().size() != nlevels || ex.u_max().size() != 16 ||
        ex.bit_pattern().size() != 512)
        cv::ref_shim_abort("ref_tables: unexpected table size");
    for (int i = 0; i < nlevels; ++i) {
        scale[i] = a[i], inv_scale[i] = b[i], sigma2[i] = c[i], inv_sigma2[i] = d[i];
        features_per_level[i] = ex.features_per_level()[i];
    }
    for (int i = 0; i < 16; ++i) umax16[i] = ex.u_max()[i];
    for (int i = 0; i < 512; ++i) pattern[2 * i] = ex.bit_pattern()[i].x, pattern[2 * i + 1] = ex.bit_pattern()[i].y;
}

}  // extern "C"
