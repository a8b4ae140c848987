// ref_cv.hpp -- TEST INFRASTRUCTURE ONLY.
//
// The slice of the OpenCV API that the reference's ORBextractor_old.cc names, written for this
// project so that the reference file compiles unchanged (oracle/ref/README.md).  Containers and
// rounding helpers are implemented here; the four image primitives (FAST, GaussianBlur,
// fastAtan2 and, through the accelerator stand-in, resize) are declared here and defined in
// ref_glue.cpp, where they delegate to liborb_oracle.so.
#pragma once
#include <algorithm>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <iterator>
#include <list>
#include <memory>
#include <utility>
#include <vector>

typedef unsigned char uchar;

#define CV_PI 3.1415926535897932384626433832795
#define CV_8U 0
#define CV_8UC1 0

// round half to even (the SSE2 / lrint form OpenCV builds on x86-64 and aarch64)
inline int cvRound(double v) { return (int)lrint(v); }
inline int cvRound(float v) { return (int)lrintf(v); }
inline int cvRound(int v) { return v; }
inline int cvFloor(double v) { int i = (int)v; return i - (i > v); }
inline int cvFloor(float v) { int i = (int)v; return i - (i > v); }
inline int cvCeil(double v) { int i = (int)v; return i + (i < v); }
inline int cvCeil(float v) { int i = (int)v; return i + (i < v); }

namespace cv {

[[noreturn]] inline void ref_shim_abort(const char* what) {
    fprintf(stderr, "ref shim: %s\n", what);
    abort();
}

enum { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_WRAP = 3,
       BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4, BORDER_ISOLATED = 16 };
enum { INTER_NEAREST = 0, INTER_LINEAR = 1, INTER_CUBIC = 2, INTER_AREA = 3 };

template <typename T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T _x, T _y) : x(_x), y(_y) {}
    Point_& operator*=(float s) {
        x = (T)(x * s);
        y = (T)(y * s);
        return *this;
    }
};
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<float> Point2f;

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

struct KeyPoint {
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
    KeyPoint() : pt(0, 0), size(0), angle(-1), response(0), octave(0), class_id(-1) {}
};

// Single-channel 8-bit matrix: a view (rows, cols, step) on a reference-counted buffer, or on
// memory the caller owns.  Every allocation holds exactly rows * cols bytes, so a read past the
// last row or before the first leaves the allocation (the sanitized self-test relies on that).
class Mat {
public:
    int rows, cols;
    size_t step;
    uchar* data;

    Mat() : rows(0), cols(0), step(0), data(nullptr) {}
    Mat(int r, int c, int type) : Mat() { create(r, c, type); }
    Mat(Size s, int type) : Mat() { create(s.height, s.width, type); }
    Mat(int r, int c, int type, void* ext, size_t st = 0)
        : rows(r), cols(c), step(st ? st : (size_t)c), data((uchar*)ext) {
        if (type != CV_8UC1) ref_shim_abort("Mat: only CV_8UC1");
    }

    void create(int r, int c, int type) {
        if (type != CV_8UC1) ref_shim_abort("Mat: only CV_8UC1");
        if (data && r == rows && c == cols) return;
        buf_ = std::make_shared<std::vector<uchar>>((size_t)r * c);
        rows = r, cols = c, step = (size_t)c, data = buf_->data();
    }
    void release() {
        buf_.reset();
        rows = cols = 0, step = 0, data = nullptr;
    }
    static Mat zeros(int r, int c, int type) {
        Mat m(r, c, type);
        if (m.data) memset(m.data, 0, (size_t)r * c);
        return m;
    }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    int type() const { return CV_8UC1; }
    size_t step1() const { return step; }

    template <typename T> T& at(int r, int c) {
        static_assert(sizeof(T) == 1, "Mat: 8-bit only");
        return *(T*)(data + (size_t)r * step + c);
    }
    template <typename T> const T& at(int r, int c) const {
        static_assert(sizeof(T) == 1, "Mat: 8-bit only");
        return *(const T*)(data + (size_t)r * step + c);
    }
    uchar* ptr(int r = 0) { return data + (size_t)r * step; }
    const uchar* ptr(int r = 0) const { return data + (size_t)r * step; }

    Mat rowRange(int r0, int r1) const {
        if (r0 < 0 || r1 < r0 || r1 > rows) ref_shim_abort("rowRange out of range");
        Mat m(*this);
        m.rows = r1 - r0, m.data = data + (size_t)r0 * step;
        return m;
    }
    Mat colRange(int c0, int c1) const {
        if (c0 < 0 || c1 < c0 || c1 > cols) ref_shim_abort("colRange out of range");
        Mat m(*this);
        m.cols = c1 - c0, m.data = data + c0;
        return m;
    }
    Mat row(int r) const { return rowRange(r, r + 1); }
    Mat clone() const {
        Mat m;
        if (empty()) return m;
        m.create(rows, cols, CV_8UC1);
        for (int r = 0; r < rows; ++r) memcpy(m.ptr(r), ptr(r), (size_t)cols);
        return m;
    }
    // dst is a header on shared pixels (descriptors.row(i)): same size required, as create()
    // would be a no-op there
    void copyTo(const Mat& dst) const {
        if (dst.rows != rows || dst.cols != cols || !dst.data) ref_shim_abort("copyTo: size mismatch");
        for (int r = 0; r < rows; ++r) memcpy(dst.data + (size_t)r * dst.step, ptr(r), (size_t)cols);
    }

private:
    std::shared_ptr<std::vector<uchar>> buf_;
};

class _InputArray {
public:
    _InputArray(const Mat& m) : m_(&m) {}
    bool empty() const { return m_->empty(); }
    Mat getMat() const { return *m_; }

private:
    const Mat* m_;
};
class _OutputArray {
public:
    _OutputArray(Mat& m) : m_(&m) {}
    void release() const { m_->release(); }
    void create(int r, int c, int type) const { m_->create(r, c, type); }
    Mat getMat() const { return *m_; }

private:
    Mat* m_;
};
typedef const _InputArray& InputArray;
typedef const _OutputArray& OutputArray;

// defined in ref_glue.cpp on the oracle's primitives
void FAST(const Mat& image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmaxSuppression);
void GaussianBlur(const Mat& src, Mat& dst, Size ksize, double sigmaX, double sigmaY, int borderType);
float fastAtan2(float y, float x);

// named only by ComputeKeyPointsOld, which nothing calls
struct KeyPointsFilter {
    static void retainBest(std::vector<KeyPoint>&, int) { ref_shim_abort("KeyPointsFilter::retainBest reached"); }
};

}  // namespace cv
