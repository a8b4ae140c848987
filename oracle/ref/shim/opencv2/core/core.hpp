// stand-in for the OpenCV header of this name (oracle/ref/README.md)
#pragma once
#include "../ref_cv.hpp"
