// VolumeLoader.h -- voxel volumes of the host API: MetaImage headers (.mhd, the
// format ITK, 3D Slicer and most phantom distributions write) with their raw
// data file beside them.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

// A labelled volume as xrt_upload_volume takes it: labels[(z * ny + y) * nx +
// x] (0: empty, L into plane L - 1), an optional density of the same shape
// (empty: 1), dims = {nx, ny, nz}, the minimum corner of voxel (0, 0, 0) and
// the voxel's size, in x, y, z order.
struct Volume {
    std::vector<unsigned char> labels;
    std::vector<float> density;
    unsigned dims[3] = {0, 0, 0};
    float origin[3] = {0.0f, 0.0f, 0.0f};
    float spacing[3] = {1.0f, 1.0f, 1.0f};
    unsigned num_labels = 0;           // the largest label
};

// What the loaders throw: code is XRT_ERR_IO (a file cannot be read) or
// XRT_ERR_FORMAT (the header's key named in what() is missing, malformed or
// holds something this loader refuses).
struct VolumeError : std::runtime_error {
    int code;
    VolumeError(int code, const std::string& what) : std::runtime_error(what), code(code) {}
};

// One MetaImage: the header's geometry and its data, u8 (MET_UCHAR) or f32
// (MET_FLOAT) -- the other vector stays empty.
struct MetaImage {
    unsigned dims[3] = {0, 0, 0};
    float origin[3] = {0.0f, 0.0f, 0.0f};
    float spacing[3] = {1.0f, 1.0f, 1.0f};
    std::vector<unsigned char> u8;
    std::vector<float> f32;
};

// Reads a header and its data file.  Needs NDims = 3, DimSize, ElementSpacing,
// ElementType = MET_UCHAR or MET_FLOAT and ElementDataFile = NAME (resolved
// beside the header; the last key); Offset (or Origin, or Position) defaults
// to 0 0 0.  Refuses CompressedData = True, another element type or channel
// count, a TransformMatrix (or Rotation, or Orientation) that is not the
// identity, ElementByteOrderMSB or BinaryDataByteOrderMSB = True, BinaryData =
// False, a HeaderSize other than 0, data inside the header (LOCAL) or in
// slices (LIST), and a data file shorter than the volume.  Other keys are
// ignored.
MetaImage loadMetaImage(const std::string& path);

// The labels of a MET_UCHAR file into `volume` (replacing it; no density), and
// a MET_FLOAT file of the same dims as volume's density.
void loadVolume(const std::string& path, Volume& volume);
void loadVolumeDensity(const std::string& path, Volume& volume);

// Writes a f32 volume (data[(z * ny + y) * nx + x], dims = {nx, ny, nz}, the
// minimum corner of voxel (0, 0, 0) and the voxel's size) as `path` -- a .mhd
// header with ElementType = MET_FLOAT, uncompressed -- and its raw
// little-endian data in NAME.raw beside it: what loadMetaImage (and
// loadVolumeDensity) reads back bit for bit, a reconstruction's way out.
// Throws VolumeError: XRT_ERR_ARGUMENT for a path that does not end in .mhd, a
// size outside 1..2048 or a spacing that is not above 0, XRT_ERR_IO when a file
// cannot be written.
void saveVolume(const std::string& path, const unsigned dims[3], const float origin[3], const float spacing[3],
                const float* data);
// The same for u8 labels, ElementType = MET_UCHAR: what loadVolume reads back, a voxelised scene's way out.
void saveVolume(const std::string& path, const unsigned dims[3], const float origin[3], const float spacing[3],
                const unsigned char* labels);
