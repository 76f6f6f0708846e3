// VolumeLoader.cpp -- see VolumeLoader.h.
#include "VolumeLoader.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <limits>
#include <sstream>

#include "xrt.h"

namespace {

std::string trimmed(const std::string& s)
{
    size_t a = 0, b = s.size();
    while (a < b && std::isspace((unsigned char)s[a])) ++a;
    while (b > a && std::isspace((unsigned char)s[b - 1])) --b;
    return s.substr(a, b - a);
}

[[noreturn]] void refuse(const std::string& path, const std::string& key, const std::string& why)
{
    throw VolumeError(XRT_ERR_FORMAT, path + ": " + key + ": " + why);
}

// `count` finite numbers, and nothing else.
std::vector<double> numbers(const std::string& path, const std::string& key, const std::string& value, size_t count)
{
    std::istringstream in(value);
    std::vector<double> out;
    std::string f;
    while (in >> f) {
        size_t used = 0;
        double v = 0.0;
        try {
            v = std::stod(f, &used);
        } catch (const std::exception&) {
            used = 0;
        }
        if (used != f.size() || !std::isfinite(v)) refuse(path, key, "'" + f + "' is not a finite number");
        out.push_back(v);
    }
    if (out.size() != count)
        refuse(path, key, std::to_string(out.size()) + " values, " + std::to_string(count) + " expected");
    return out;
}

bool is_true(const std::string& v) { return v == "True" || v == "true" || v == "TRUE" || v == "1"; }

}  // namespace

MetaImage loadMetaImage(const std::string& path)
{
    std::ifstream in(path);
    if (!in) throw VolumeError(XRT_ERR_IO, "Cannot open the file " + path);
    MetaImage img;
    bool have_ndims = false, have_dims = false, have_spacing = false;
    std::string type, data_file, line;
    while (data_file.empty() && std::getline(in, line)) {
        const size_t eq = line.find('=');
        if (eq == std::string::npos) {
            if (trimmed(line).empty()) continue;
            refuse(path, trimmed(line), "not a 'Key = Value' line");
        }
        const std::string key = trimmed(line.substr(0, eq)), value = trimmed(line.substr(eq + 1));
        if (key == "NDims") {
            if (numbers(path, key, value, 1)[0] != 3.0) refuse(path, key, "only 3 is read");
            have_ndims = true;
        } else if (key == "DimSize") {
            const std::vector<double> v = numbers(path, key, value, 3);
            for (int a = 0; a < 3; ++a) {
                if (v[a] < 1.0 || v[a] > 2048.0 || v[a] != std::floor(v[a])) refuse(path, key, "a size is not 1 to 2048");
                img.dims[a] = (unsigned)v[a];
            }
            have_dims = true;
        } else if (key == "ElementSpacing") {
            const std::vector<double> v = numbers(path, key, value, 3);
            for (int a = 0; a < 3; ++a) {
                img.spacing[a] = (float)v[a];
                if (!(img.spacing[a] > 0.0f) || !std::isfinite(img.spacing[a])) refuse(path, key, "a spacing is not above 0");
            }
            have_spacing = true;
        } else if (key == "Offset" || key == "Origin" || key == "Position") {
            const std::vector<double> v = numbers(path, key, value, 3);
            for (int a = 0; a < 3; ++a) img.origin[a] = (float)v[a];
        } else if (key == "TransformMatrix" || key == "Rotation" || key == "Orientation") {
            const std::vector<double> v = numbers(path, key, value, 9);
            for (int k = 0; k < 9; ++k)
                if (v[k] != (k % 4 == 0 ? 1.0 : 0.0)) refuse(path, key, "only the identity is read (the volume has no pose)");
        } else if (key == "CompressedData") {
            if (is_true(value)) refuse(path, key, "compressed data is not read");
        } else if (key == "ElementByteOrderMSB" || key == "BinaryDataByteOrderMSB") {
            if (is_true(value)) refuse(path, key, "big-endian data is not read");
        } else if (key == "BinaryData") {
            if (!is_true(value)) refuse(path, key, "text data is not read");
        } else if (key == "ElementNumberOfChannels") {
            if (numbers(path, key, value, 1)[0] != 1.0) refuse(path, key, "only 1 is read");
        } else if (key == "HeaderSize") {
            if (numbers(path, key, value, 1)[0] != 0.0) refuse(path, key, "only 0 is read");
        } else if (key == "ElementType") {
            if (value != "MET_UCHAR" && value != "MET_FLOAT") refuse(path, key, value + " is not MET_UCHAR or MET_FLOAT");
            type = value;
        } else if (key == "ElementDataFile") {
            if (value.empty() || value == "LOCAL" || value == "LIST" || value.find('%') != std::string::npos)
                refuse(path, key, "'" + value + "' is not one raw file beside the header");
            data_file = value;
        }
    }
    if (!have_ndims) refuse(path, "NDims", "missing");
    if (!have_dims) refuse(path, "DimSize", "missing");
    if (!have_spacing) refuse(path, "ElementSpacing", "missing");
    if (type.empty()) refuse(path, "ElementType", "missing");
    if (data_file.empty()) refuse(path, "ElementDataFile", "missing");
    const size_t slash = path.find_last_of('/');
    const std::string raw = data_file[0] == '/' || slash == std::string::npos ? data_file : path.substr(0, slash + 1) + data_file;
    std::ifstream data(raw, std::ios::binary);
    if (!data) throw VolumeError(XRT_ERR_IO, path + ": ElementDataFile: cannot open the file " + raw);
    const size_t n = (size_t)img.dims[0] * img.dims[1] * img.dims[2];
    if (type == "MET_UCHAR") {
        img.u8.resize(n);
        data.read(reinterpret_cast<char*>(img.u8.data()), (std::streamsize)n);
    } else {
        img.f32.resize(n);
        data.read(reinterpret_cast<char*>(img.f32.data()), (std::streamsize)(n * sizeof(float)));
    }
    const size_t want = type == "MET_UCHAR" ? n : n * sizeof(float);
    if ((size_t)data.gcount() != want)
        refuse(path, "ElementDataFile", raw + " holds " + std::to_string((size_t)data.gcount()) + " bytes, DimSize needs " +
                                            std::to_string(want));
    return img;
}

void loadVolume(const std::string& path, Volume& volume)
{
    MetaImage img = loadMetaImage(path);
    if (img.u8.empty()) refuse(path, "ElementType", "labels are MET_UCHAR");
    volume = Volume();
    std::copy(img.dims, img.dims + 3, volume.dims);
    std::copy(img.origin, img.origin + 3, volume.origin);
    std::copy(img.spacing, img.spacing + 3, volume.spacing);
    volume.num_labels = *std::max_element(img.u8.begin(), img.u8.end());
    volume.labels = std::move(img.u8);
}

void loadVolumeDensity(const std::string& path, Volume& volume)
{
    MetaImage img = loadMetaImage(path);
    if (img.f32.empty()) refuse(path, "ElementType", "a density is MET_FLOAT");
    if (!std::equal(img.dims, img.dims + 3, volume.dims))
        refuse(path, "DimSize", std::to_string(img.dims[0]) + " " + std::to_string(img.dims[1]) + " " +
                                    std::to_string(img.dims[2]) + " differs from the labels' " +
                                    std::to_string(volume.dims[0]) + " " + std::to_string(volume.dims[1]) + " " +
                                    std::to_string(volume.dims[2]));
    volume.density = std::move(img.f32);
}

namespace {

// A MetaImage header and its raw file: `data` holds dims' voxels of `bytes` bytes each, of ElementType `type`.
void saveMetaImage(const std::string& path, const unsigned dims[3], const float origin[3], const float spacing[3],
                   const void* data, size_t bytes, const char* type)
{
    if (path.size() < 5 || path.compare(path.size() - 4, 4, ".mhd") != 0)
        throw VolumeError(XRT_ERR_ARGUMENT, path + ": a volume is written as NAME.mhd");
    if (!dims || !origin || !spacing || !data) throw VolumeError(XRT_ERR_ARGUMENT, path + ": NULL argument");
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 1u || dims[a] > 2048u) throw VolumeError(XRT_ERR_ARGUMENT, path + ": a size is not 1 to 2048");
        if (!(spacing[a] > 0.0f) || !std::isfinite(spacing[a]) || !std::isfinite(origin[a]))
            throw VolumeError(XRT_ERR_ARGUMENT, path + ": a spacing is not above 0 or the origin is not finite");
    }
    const std::string raw = path.substr(0, path.size() - 4) + ".raw";
    const size_t slash = raw.find_last_of('/');
    {
        std::ofstream out(raw, std::ios::binary);
        out.write(static_cast<const char*>(data), (std::streamsize)((size_t)dims[0] * dims[1] * dims[2] * bytes));
        if (!out) throw VolumeError(XRT_ERR_IO, "Cannot write the file " + raw);
    }
    std::ofstream head(path);
    head << std::setprecision(std::numeric_limits<float>::max_digits10);         // (a f32 survives the text)
    head << "ObjectType = Image\nNDims = 3\nBinaryData = True\nBinaryDataByteOrderMSB = False\nCompressedData = False\n"
         << "TransformMatrix = 1 0 0 0 1 0 0 0 1\n"
         << "Offset = " << origin[0] << ' ' << origin[1] << ' ' << origin[2] << "\n"
         << "ElementSpacing = " << spacing[0] << ' ' << spacing[1] << ' ' << spacing[2] << "\n"
         << "DimSize = " << dims[0] << ' ' << dims[1] << ' ' << dims[2] << "\n"
         << "ElementType = " << type << "\n"
         << "ElementDataFile = " << (slash == std::string::npos ? raw : raw.substr(slash + 1)) << "\n";
    head.close();
    if (!head) throw VolumeError(XRT_ERR_IO, "Cannot write the file " + path);
}

}  // namespace

void saveVolume(const std::string& path, const unsigned dims[3], const float origin[3], const float spacing[3],
                const float* data)
{
    saveMetaImage(path, dims, origin, spacing, data, sizeof(float), "MET_FLOAT");
}

void saveVolume(const std::string& path, const unsigned dims[3], const float origin[3], const float spacing[3],
                const unsigned char* labels)
{
    saveMetaImage(path, dims, origin, spacing, labels, 1u, "MET_UCHAR");
}
