// Output formatting after the hot path: colour-coded flow image (binary PPM) and magnitude raw.
// Interface of the reference's src/utils/io_utils.h:31-79; byte-compatible output
// (io_utils.cpp:35-114,140-225: "P6 \n<nx> <ny> \n255\n" header, Bruhn colour wheel).
#pragma once

#include <string>

#include "data2d.h"

namespace IOUtils {

typedef unsigned char GRAY;

struct RGBColor {
    int r = 0, g = 0, b = 0;
    RGBColor() = default;
    RGBColor(int red, int green, int blue) : r(red), g(green), b(blue) {}
};

// exit(255) when the file cannot be opened, like the reference (io_utils.cpp:47-51,88-92).
void WriteFlowToImageRGB(Data2D& u, Data2D& v, float flowMaxScale, std::string fileName);
void WriteMagnitudeToFileF32(Data2D& u, Data2D& v, std::string fileName);
// An occlusion mask as a binary greyscale image (P5, "P5\n<nx> <ny>\n255\n"): 255 where the mask is non-zero, 0 elsewhere.
// No reference counterpart; exit(255) when the file cannot be opened, like the writers above.
void WriteMaskToImagePGM(Data2D& mask, std::string fileName);

// Middlebury .flo (Baker et al., IJCV 2011): the float magic 202021.25 ("PIEH"), int32 width, int32 height, then width * height
// interleaved little-endian float32 (u, v) pairs in row-major order.  No reference counterpart.  ReadFlowFLO refuses -- false,
// u and v left as they were -- a file it cannot open, a bad magic, a size outside 1 .. kFloMaxSide per side or beyond
// kFloMaxPixels in all, and a file shorter than its header says (checked before any sample is read); trailing bytes are
// ignored.  WriteFlowFLO returns false when the file cannot be written or u and v differ in size.
constexpr size_t kFloMaxSide = size_t(1) << 20;
constexpr size_t kFloMaxPixels = size_t(1) << 28;
bool ReadFlowFLO(const std::string& fileName, Data2D& u, Data2D& v);
bool WriteFlowFLO(Data2D& u, Data2D& v, const std::string& fileName);

// Direction -> hue, magnitude (clipped at 1) -> brightness.
RGBColor ConvertToRGB(float x, float y);

inline int ConvertToByte(int num) { return num >= 255 ? 255 : (num > 0 ? num : 0); }

inline GRAY ConvertToGray(float number)
{
    if (number < 0.0f) return 0;
    if (number > 255.0f) return 255;
    return static_cast<GRAY>(number);
}

}  // namespace IOUtils
