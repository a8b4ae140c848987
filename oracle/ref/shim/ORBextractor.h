// ORBextractor.h -- TEST INFRASTRUCTURE ONLY.
//
// What the reference's ORBextractor_old.cc includes under this name.  It declares the Android and
// accelerator names that file uses (defined in ref_glue.cpp), then includes the generated copy of
// the reference's own class declaration (oracle/_ref/gen/, never committed).
#pragma once
#include <cstdint>
#include <vector>

#include <opencv2/opencv.hpp>

// AHardwareBuffer: only the second operator() overload touches it; nothing here calls that
// overload, and the stubs abort if they are reached.
struct AHardwareBuffer;
struct AHardwareBuffer_Desc {
    uint32_t width, height, layers, format;
    uint64_t usage;
    uint32_t stride, rfu0;
    uint64_t rfu1;
};
enum { AHARDWAREBUFFER_USAGE_CPU_READ_OFTEN = 3 };
void AHardwareBuffer_describe(const AHardwareBuffer* buffer, AHardwareBuffer_Desc* desc);
int AHardwareBuffer_lock(AHardwareBuffer* buffer, uint64_t usage, int32_t fence, const void* rect, void** out);
int AHardwareBuffer_unlock(AHardwareBuffer* buffer, int32_t* fence);

struct FrameAHB {
    static int s_HardwareBufferUses;
};

// The reference calls these two accelerator methods.  ComputePyramid builds the canonical pyramid
// (the level sizes of the loop the reference keeps commented out) on the oracle's resize; the
// ten-argument ComputeKeyPointsOctTree belongs to the AHardwareBuffer overload and aborts.
class LynxHardwareAccelerator {
public:
    static LynxHardwareAccelerator& GetInstance();
    void ComputePyramid(const cv::Mat& image, int nlevels, const std::vector<float>& invScaleFactor,
                        std::vector<cv::Mat>& pyramid);
    void ComputeKeyPointsOctTree(std::vector<std::vector<cv::KeyPoint>>& allKeypoints,
                                 std::vector<cv::Mat>& pyramid, int eye, int nfeatures, int nlevels,
                                 int iniThFAST, int minThFAST, std::vector<int>& featuresPerLevel,
                                 std::vector<float>& scaleFactor, std::vector<int>& umax);
};

#include "ORBextractor_old.h"
