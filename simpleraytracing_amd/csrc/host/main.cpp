// main.cpp -- xrt_main: the reference's command line (src/main.cxx:182-392)
// over the MI355X render path.
//
//   -h, --help                 usage
//   -s, --size W H             image size (default 2048 2048)
//   -b, --background R G B     parsed and unused, as in the reference
//   -f, --filename NAME        output text file "./out/NAME" (default test.jpg,
//                              which, as in the reference, receives text)
//   -i, --input FILE           mesh file (default ./dragon.ply); repeatable: the
//                              files' meshes make one scene, in order
// additions:
//   -g, --gpus N               row strips over N GPUs (default 1)
//   -k, --kernel brute|tiled|binned  render kernel (default: automatic -- tiled
//                              for small frames, binned past 2e7 footprint tests)
//   -t, --threads N            accepted for main-pthreads*.cxx compatibility (ignored)
//       --signed               the L-buffer fork (main-pthreads-lbuffer.cxx): signed
//                              multi-material L-buffer + hole fill
//       --materials MU0,MU1,.. the materials model: every mesh attenuates with its
//                              own coefficient (one value per loaded mesh) + hole fill
//       --spectrum FILE        the spectrum model: a polychromatic beam.  FILE is
//                              text, '#' starts a comment; the first data line holds
//                              the K bin weights, each further line one mesh's K
//                              coefficients, in load order + hole fill
//       --paths                the paths model: trace once and write every mesh's plane
//                              of signed path lengths to NAME.m<m>.EXT and the mask
//                              of open meshes to NAME.open.EXT (-f NAME.EXT); with
//                              --spectrum FILE the table is then applied to the planes
//                              and NAME.EXT is what --spectrum FILE alone writes
//       --pose M=v0,...,v11    mesh M (load order, from 0) under a pose: 12 values, a
//                              row-major 3x4 [R | t] (the fork's transformMatrix and a
//                              translation), applied on the device; repeatable, once
//                              per mesh
//       --turntable N[:x|y|z][:M,M,...]  N projections: projection k has the listed
//                              meshes (every mesh when none is listed) turned k*360/N
//                              degrees about the axis (default y, the fork's rotateMat)
//                              through the rest scene's box centre, under the rest
//                              scene's camera, and is written to NAME.pKKK.EXT (so are
//                              --lbuffer's and --u8's files)
//       --lsf FILE             the detector's line-spread function over the image that
//                              NAME.EXT and --u8 receive (every model; every projection
//                              of --turntable; with --paths, --spectrum's image).  FILE
//                              is text as --spectrum's: the first data line holds the
//                              taps along x, an optional second line those along y (one
//                              line: both axes); an odd count, at most 129; applied as
//                              written (a correlation), edges replicated, not normalised.
//                              --lbuffer, NAME.m<m> and NAME.open stay as rendered
//       --lsf-gaussian SIGMA[:TAPS]  the same with a normalised Gaussian of SIGMA pixels
//                              on both axes, TAPS (odd) defaulting to 2*ceil(4*SIGMA)+1,
//                              at most 129
//       --log-projection I0    line integrals: the image that NAME.EXT receives becomes
//                              -ln(I / I0), I0 finite and > 0 (80 is these models'
//                              unattenuated intensity), after --lsf when both are
//                              given (the detector blurs intensity); every model, every
//                              projection of --turntable.  --u8, --lbuffer, NAME.m<m>
//                              and NAME.open stay as rendered
//       --reconstruct FILE.mhd[:N]  with --turntable N and --log-projection: the scan's line
//                              integrals reconstructed by FDK (the ramp filter and the
//                              cone-beam backprojector on the device) into an N x N x N grid
//                              (default 128; 1 to 2048) of float32 attenuation per scene
//                              length unit, a cube about the turntable's centre whose side
//                              is the scene box's diagonal, written as FILE.mhd (MetaImage,
//                              MET_FLOAT) and FILE.raw beside it.  The turntable must turn
//                              every mesh about an axis parallel to the detector's up (--turntable N:z):
//                              another axis is refused once the meshes are loaded and the
//                              camera is known, before a projection is rendered.
//       --voxelize FILE.mhd[:N]  the scene voxelised on the device on exactly the
//                              grid --reconstruct FILE.mhd[:N] uses: FILE.mhd (MetaImage,
//                              MET_UCHAR) and FILE.raw hold 0 outside every mesh, else 1 + the
//                              last mesh the voxel's centre lies in -- a --volume phantom, and
//                              the truth a reconstruction of the same N is compared with voxel
//                              by voxel.  With --materials also FILE.mu.mhd (MET_FLOAT): the
//                              sum of the coefficients of the meshes each voxel lies in.  The
//                              meshes stand under --pose's poses, those --turntable turns at
//                              rest (its projection 0).  Valid without --turntable: the cube's
//                              centre is the loaded scene's box centre either way, which is the
//                              turntable's.
//       --sirt K[:S[:RELAX]]   with --reconstruct: reconstruct by K iterations of SIRT (S = 1,
//                              the default) or OS-SART over S subsets (1 to 64, at most the
//                              projections; subset s holds the projections p with p mod S
//                              == s) instead of FDK, from zeros, every update relaxed by
//                              RELAX (default 1) and kept >= 0.  The same cube and the same
//                              refusals as FDK's.
//       --mltr K[:S[:RELAX]]   with --reconstruct, in the place of --sirt: K iterations of
//                              OS-MLTR, the maximum-likelihood solver for
//                              transmission counts.  It is given each projection's intensity as
//                              it stands just before the logarithm -- after --scatter, --lsf
//                              and --noise; zero counts are fine --, a flat field of I0 and,
//                              with --scatter, each projection's scatter estimate as the
//                              background; FILE.counts.mhd (and FILE.background.mhd) keep
//                              those planes.  NAME.EXT receives what --log-projection writes.
//       --tv STEPS[:ALPHA[:REDUCTION[:EPS]]]
//                              with --sirt or --mltr: after every iteration STEPS descent steps on the
//                              volume's total variation, each ALPHA (default
//                              0.2) times as long as the distance the iteration moved the
//                              volume; ALPHA is multiplied by REDUCTION (default 1, in
//                              (0, 1]) after every iteration and EPS (default 1e-8) smooths
//                              the norm.  It flattens noise and keeps edges; ALPHA above
//                              about 0.5 flattens the object's level too.
//       --sinogram FILE        with --turntable N and --log-projection: also write the N
//                              projections' line integrals as one sinogram per detector
//                              row, raw little-endian f32 in (height, N, width) order
//       --noise GAIN[:SEED]    photon noise: every pixel of the image that NAME.EXT
//                              receives becomes a Poisson count of mean I * GAIN (GAIN
//                              photons per unit of image value, finite and > 0), divided
//                              by GAIN again; after --lsf and before --log-projection
//                              (and --sinogram).  SEED (unsigned, 64 bits) defaults to
//                              0; projection p of --turntable draws the noise of pixels
//                              p*W*H onwards, as one call over the stacked scan would.
//                              Refused where --lsf is.  --u8, --lbuffer, NAME.m<m> and
//                              NAME.open stay as rendered
//       --supersample B        pixel-area integration: every projection is rendered at
//                              W*B x H*B pixels (B in 1..8; -s W H stays the size of
//                              what is written) and each written pixel is the mean of
//                              the B x B samples that tile its area, summed in f64 on
//                              the device.  B a power of two samples at the centres
//                              spacing/B apart exactly; for another B the finer frame's
//                              spacing is renderLoop's own for W*B x H*B, which may
//                              differ from spacing/B by an ulp
//       --focal-spot UxV[:NUxNV]  a finite focal spot: a uniform rectangle of U (along the
//                              detector's "right") by V (along "up") scene units, finite
//                              and >= 0, sampled at the centres of an NU x NV grid
//                              (default 3x3, NU*NV <= 64); every projection is rendered
//                              from each sub-source -- the detector does not move -- and
//                              the renders are averaged with --supersample's samples.
//                              With either option every model (default, --signed,
//                              --materials, --spectrum; the model's hole fill on each
//                              sample) and every --turntable projection, with --pose;
//                              NAME.EXT and --u8 receive the integrated image, and --lsf,
//                              --noise (first_index p*W*H of the written size),
//                              --log-projection and --sinogram follow in their order.
//                              Refused with -g N, --rows, --batch, --paths and --lbuffer
//                              (an integrated frame has no single L-buffer)
//       --detector FILE        the spectral detector, with --paths --spectrum FILE2: per
//                              pixel and energy bin a photon count, summed into energy
//                              channels.  FILE is text: one line of K responses (finite,
//                              >= 0) per channel, at most 8 ('#' starts a comment); a
//                              line of bin energies is an energy-integrating panel, lines
//                              of 0/1 windows a photon-counting detector.  Writes
//                              NAME.c<c>.EXT per channel, after the model's hole fill;
//                              NAME.EXT stays what --paths --spectrum writes.  Without
//                              --noise: the expected values at gain 1.  With --noise
//                              GAIN[:SEED] the draw happens inside the detector, a count
//                              per bin, and the channels are divided by GAIN; projection
//                              p of --turntable draws the noise of pixels p*W*H onwards.
//                              Not with --lsf, --lsf-gaussian, --log-projection,
//                              --sinogram, --supersample, --focal-spot, -g, --rows, --batch
//       --scatter FILE         the scatter model, with --paths --spectrum FILE2: a kernel-
//                              superposition estimate of scattered radiation added to
//                              the image.  FILE is text ('#' starts a comment): a line
//                              with the binning factor D (a power of two, 1 to 64), one
//                              line of K coefficients (finite, >= 0) per mesh -- the part
//                              of --spectrum's coefficient that scatters --, then one to
//                              four lines AMP SIGMA_PIXELS[:TAPS], a Gaussian scatter
//                              kernel each (TAPS on the binned grid, odd, default
//                              2*ceil(4*SIGMA/D)+1, at most 129).  Runs after the hole
//                              fill and before --lsf, --noise and --log-projection, per
//                              projection of --turntable (and so under --reconstruct).
//                              NAME.EXT and --u8 receive the total, NAME.scatter.EXT the
//                              scatter alone.  Not with --detector, --supersample,
//                              --focal-spot, --volume, -g, --rows, --batch
//       --read-noise SIGMA     with --detector and --noise: additive Gaussian (electronic)
//                              noise of SIGMA counts (finite, >= 0) on every channel
//       --decompose BASIS[:ITER[:TOL]]  with --detector: material decomposition of the
//                              channels as written (the text files' six significant
//                              digits, after the hole fill, as intensities under the
//                              detector's gain), so that the files on disk reproduce it.
//                              BASIS is text: one line of K coefficients (finite, >= 0)
//                              per basis material, 1 to 3 lines ('#' starts a comment), K
//                              the spectrum's bins; at most ITER iterations a pixel
//                              (1 to 200, default 32) until no line integral moves by
//                              more than TOL (default 1e-6), from xrt_decompose_guess'
//                              start.  Writes NAME.b<b>.EXT per basis material, after the
//                              channels, and prints the number of pixels that failed or
//                              ran ITER iterations.  Not with -g N
//       --volume FILE.mhd      with --paths: a voxel phantom beside the meshes (or alone:
//                              -i may then be omitted).  FILE.mhd is a MetaImage header
//                              of MET_UCHAR labels (0: empty) with its raw file beside
//                              it.  The camera is fitted to the union of the scene's box
//                              and the volume's; label L's plane of path lengths is
//                              written to NAME.m<k>.EXT behind the meshes' (k = meshes +
//                              L - 1), and --spectrum's table holds one row per mesh,
//                              then one per label.  The volume has no pose.  Not with
//                              -g, --rows, --batch, --supersample, --focal-spot,
//                              --turntable, --pose
//       --volume-density FILE.mhd  with --volume: a MET_FLOAT density per voxel, of the
//                              volume's dims; a segment counts times its voxel's density
//       --lbuffer FILE         also write the L-buffer as raw little-endian f32
//       --u8 FILE              also write the 8-bit image (LUT 0..80) as PGM
//       --time                 print render wall-clock and Mrays/s
//       --rows A:B             render image rows [A, B) only and write that
//                              strip (B - A text rows), as one pthreads
//                              thread's share of the frame
//       --batch N              render the frame N times back to back (one
//                              xrt_render_frames call) and write the last;
//                              with --time, the device time per frame
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "Image.h"
#include "RayTracer.h"
#include "TriangleMesh.h"
#include "xrt.h"

namespace {

void showUsage(const std::string& prog)
{
    std::cerr << "Usage: " << prog << " <option(s)>\n"
              << "Options:\n"
              << "\t-h,--help\t\t\tShow this help message\n"
              << "\t-s,--size IMG_WIDTH IMG_HEIGHT\tSpecify the image size in number of pixels (default values: 2048 2048)\n"
              << "\t-b,--background R G B\t\tSpecify the background colour in RGB (accepted, unused)\n"
              << "\t-f,--filename FILENAME\t\tName of the output text file, written to ./out/ (default: test.jpg)\n"
              << "\t-i,--input FILENAME\t\tInput mesh, PLY or OBJ (default: ./dragon.ply); repeat for a scene of several files\n"
              << "\t-g,--gpus N\t\t\tRender row strips on N GPUs (default: 1)\n"
              << "\t-k,--kernel brute|tiled|binned\tRender kernel (default: automatic)\n"
              << "\t--signed\t\t\tSigned multi-material L-buffer and hole fill (main-pthreads-lbuffer.cxx)\n"
              << "\t--materials MU0,MU1,...\t\tMaterials model: one attenuation coefficient per loaded mesh, and hole fill\n"
              << "\t--spectrum FILE\t\t\tSpectrum model: FILE holds a line of K bin weights, then one line of K coefficients per loaded mesh\n"
              << "\t--paths\t\t\t\tPaths model: write each mesh's path-length plane (NAME.m<m>.EXT) and the open mask (NAME.open.EXT); with --spectrum FILE, apply it to the planes\n"
              << "\t--pose M=v0,...,v11\t\tMesh M under a pose: 12 values, row-major 3x4 [R | t]; repeat for other meshes\n"
              << "\t--turntable N[:x|y|z][:M,...]\tN projections, the listed meshes (default: all) turned k*360/N degrees about the axis (default y) through the scene's centre; writes NAME.pKKK.EXT\n"
              << "\t--lsf FILE\t\t\tDetector line-spread function over the written image: FILE holds a line of taps along x and, optionally, one along y (odd counts, at most 129)\n"
              << "\t--lsf-gaussian SIGMA[:TAPS]\tThe same with a normalised Gaussian of SIGMA pixels (TAPS odd, default 2*ceil(4*SIGMA)+1, at most 129)\n"
              << "\t--log-projection I0\t\tLine integrals: write -ln(I / I0) (I0 finite and > 0; after --lsf) instead of the intensity I; --u8 and --lbuffer stay as rendered\n"
              << "\t--sinogram FILE\t\t\tWith --turntable N and --log-projection: also write the line integrals as raw float32 sinograms, (height, N, width)\n"
              << "\t--reconstruct FILE.mhd[:N]\tWith --turntable N:z (every mesh, about the detector's up) and --log-projection: reconstruct the scan by FDK into an N^3 grid (default 128) about the turntable's centre, its side the scene box's diagonal; writes FILE.mhd (MET_FLOAT) and FILE.raw\n"
              << "\t--voxelize FILE.mhd[:N]\t\tVoxelise the scene (under --pose's poses) on the grid of --reconstruct FILE.mhd[:N]: writes FILE.mhd (MET_UCHAR, 0 or 1 + the last mesh a voxel's centre lies in) and FILE.raw, with --materials also FILE.mu.mhd (MET_FLOAT, the coefficients summed); valid without --turntable\n"
              << "\t--sirt K[:S[:RELAX]]\t\tWith --reconstruct: K iterations of SIRT (S = 1) or OS-SART over S subsets (1 to 64) instead of FDK, from zeros, relaxed by RELAX (default 1), kept >= 0\n"
              << "\t--mltr K[:S[:RELAX]]\t\tWith --reconstruct, in the place of --sirt: K iterations of OS-MLTR over S subsets, the maximum-likelihood solver for transmission counts, on each projection's intensity before the logarithm (after --scatter, --lsf, --noise), a flat field of I0 and --scatter's estimate as the background; FILE.counts.mhd keeps the planes\n"
              << "\t--tv STEPS[:ALPHA[:REDUCTION[:EPS]]]\tWith --sirt or --mltr: STEPS total-variation descent steps after every iteration, each ALPHA (default 0.2) of the iteration's move, ALPHA times REDUCTION (default 1, in (0, 1]) after every iteration, EPS (default 1e-8) under the norm; ALPHA above about 0.5 flattens the object's level\n"
              << "\t--noise GAIN[:SEED]\t\tPhoton noise on the written image: each pixel a Poisson count of mean I * GAIN, divided by GAIN (after --lsf, before --log-projection; SEED defaults to 0); --u8 and --lbuffer stay as rendered\n"
              << "\t--supersample B\t\t\tPixel-area integration: render W*B x H*B samples (B in 1..8) and write each pixel's mean over its B x B samples; -s stays the written size\n"
              << "\t--focal-spot UxV[:NUxNV]\tA finite focal spot of U x V scene units (along right and up), NU x NV sub-sources (default 3x3, at most 64), averaged on the device; not with -g, --rows, --batch, --paths, --lbuffer\n"
              << "\t--detector FILE\t\t\tSpectral detector, with --paths --spectrum: FILE holds one line of K responses per energy channel (at most 8); writes NAME.c<c>.EXT per channel; with --noise GAIN[:SEED] a Poisson count per bin, divided by GAIN, otherwise the expected values at gain 1\n"
              << "\t--scatter FILE\t\t\tScatter estimate, with --paths --spectrum: FILE holds the binning factor D (a power of two, 1 to 64), one line of K scattering coefficients per mesh, then 1 to 4 lines AMP SIGMA_PIXELS[:TAPS] (Gaussian kernels); NAME.EXT receives primary + scatter, NAME.scatter.EXT the scatter; before --lsf, --noise and --log-projection, per --turntable projection\n"
              << "\t--read-noise SIGMA\t\tWith --detector and --noise: additive Gaussian noise of SIGMA counts on every channel\n"
              << "\t--decompose BASIS[:ITER[:TOL]]\tWith --detector: material decomposition of the written channels; BASIS holds one line of K coefficients per basis material (1 to 3); at most ITER iterations a pixel (1 to 200, default 32), until no line integral moves by more than TOL (default 1e-6); writes NAME.b<b>.EXT per basis material and prints the unconverged count\n"
              << "\t--volume FILE.mhd\t\tWith --paths: a voxel phantom (MetaImage header, MET_UCHAR labels, raw file beside it) beside the meshes or alone (no -i); one plane per label behind the meshes' (NAME.m<k>.EXT), one --spectrum row per mesh, then per label; not with -g, --rows, --batch, --supersample, --focal-spot, --turntable, --pose\n"
              << "\t--volume-density FILE.mhd\tWith --volume: a MET_FLOAT density per voxel, of the volume's dims\n"
              << "\t--lbuffer FILE\t\t\tWrite the L-buffer as raw float32\n"
              << "\t--u8 FILE\t\t\tWrite the 8-bit image (0..80 keV LUT) as PGM\n"
              << "\t--time\t\t\t\tPrint render time and Mrays/s\n"
              << "\t--rows A:B\t\t\tRender and write image rows [A, B) only\n"
              << "\t--batch N\t\t\tRender the frame N times back to back, write the last\n"
              << std::endl;
}

struct Options {
    std::string output = "test.jpg";
    std::vector<std::string> inputs;
    unsigned width = 2048, height = 2048;
    int gpus = 1;
    int kernel = XRT_KERNEL_AUTO;
    std::string lbuffer, u8;
    bool time = false;
    bool signed_model = false;
    std::vector<float> materials;              // --materials: one coefficient per mesh
    bool spectrum = false;                     // --spectrum: K weights, one row of K coefficients per mesh
    std::vector<float> spectrum_weight, spectrum_mu;
    bool paths = false;                        // --paths: the per-mesh planes (and --spectrum applied to them)
    bool rows = false;
    unsigned row_begin = 0, row_end = 0;
    unsigned batch = 0;
    std::vector<std::pair<unsigned, std::array<float, 12>>> poses;   // --pose M=...: one per mesh at most
    unsigned turntable = 0;                    // --turntable: projections (0: none)
    int turn_axis = 1;                         // 0 x, 1 y, 2 z
    std::vector<unsigned> turn_meshes;         // empty: every mesh
    bool lsf_file = false, lsf_gauss = false;  // --lsf, --lsf-gaussian
    std::vector<float> lsf_x, lsf_y;           // the detector response's taps (empty: none)
    bool log_projection = false;               // --log-projection I0
    float flat_value = 0.0f;                   // I0
    std::string sinogram;                      // --sinogram FILE
    std::string reconstruct;                   // --reconstruct FILE.mhd[:N]
    unsigned reconstruct_n = 128;              // N: the grid is N x N x N
    std::string voxelize;                      // --voxelize FILE.mhd[:N]
    unsigned voxelize_n = 128;                 // N: --reconstruct's grid of that N
    unsigned sirt_iterations = 0;              // --sirt K[:S[:RELAX]] (0: FDK)
    unsigned sirt_subsets = 1;
    double sirt_relax = 1.0;
    unsigned mltr_iterations = 0;              // --mltr K[:S[:RELAX]] (0: not chosen)
    unsigned mltr_subsets = 1;
    double mltr_relax = 1.0;
    bool tv = false;                           // --tv STEPS[:ALPHA[:REDUCTION[:EPS]]]
    TVParams tv_params;
    bool noise = false;                        // --noise GAIN[:SEED]
    float noise_gain = 0.0f;
    unsigned long long noise_seed = 0;
    unsigned supersample = 0;                  // --supersample B (0: not given)
    bool focal_spot = false;                   // --focal-spot UxV[:NUxNV]
    float spot_u = 0.0f, spot_v = 0.0f;
    unsigned spot_nu = 3, spot_nv = 3;
    bool scatter = false;                      // --scatter FILE: D, a row of K coefficients per mesh, the kernels
    std::vector<std::vector<std::string>> scatter_lines;   // its data lines' fields, read once the table's size is known
    std::string scatter_file;
    ScatterModel scatter_model;
    bool detector = false;                     // --detector FILE: one row of K responses per channel
    std::vector<std::vector<float>> detector_rows;
    bool read_noise_set = false;               // --read-noise SIGMA
    float read_noise = 0.0f;
    std::string volume, volume_density;        // --volume FILE.mhd, --volume-density FILE.mhd
    bool decompose = false;                    // --decompose BASIS[:ITER[:TOL]]: one row of K coefficients per basis material
    std::vector<std::vector<float>> basis_rows;
    unsigned decompose_iter = 32;
    double decompose_tol = 1e-6;
};

// A whole, non-negative decimal number.
bool parse_index(const std::string& f, unsigned& out)
{
    if (f.empty() || f.size() > 9 || f.find_first_not_of("0123456789") != std::string::npos) return false;
    out = (unsigned)std::stoul(f);
    return true;
}

std::vector<std::string> split(const std::string& list, char sep)
{
    std::vector<std::string> out;
    for (size_t pos = 0; pos <= list.size();) {
        size_t next = list.find(sep, pos);
        if (next == std::string::npos) next = list.size();
        out.push_back(list.substr(pos, next - pos));
        pos = next + 1;
    }
    return out;
}

// --pose M=v0,...,v11
void parse_pose(const std::string& arg, Options& o)
{
    const size_t eq = arg.find('=');
    unsigned mesh = 0;
    if (eq == std::string::npos || !parse_index(arg.substr(0, eq), mesh))
        throw std::runtime_error("--pose M=v0,...,v11: '" + arg.substr(0, eq) + "' is not a mesh number");
    const std::vector<std::string> fields = split(arg.substr(eq + 1), ',');
    if (fields.size() != 12)
        throw std::runtime_error("--pose takes 12 values (a row-major 3x4 [R | t]), got " + std::to_string(fields.size()));
    std::array<float, 12> q;
    for (size_t k = 0; k < 12; ++k) {
        size_t used = 0;
        try {
            q[k] = std::stof(fields[k], &used);
        } catch (const std::exception&) {
            used = 0;
        }
        if (fields[k].empty() || used != fields[k].size() || !std::isfinite(q[k]))
            throw std::runtime_error("--pose: '" + fields[k] + "' is not a finite number");
    }
    for (const auto& have : o.poses)
        if (have.first == mesh) throw std::runtime_error("--pose given twice for mesh " + std::to_string(mesh));
    o.poses.push_back({mesh, q});
}

// --turntable N[:x|y|z][:M,M,...]
void parse_turntable(const std::string& arg, Options& o)
{
    const std::vector<std::string> parts = split(arg, ':');
    if (parts.size() > 3 || !parse_index(parts[0], o.turntable) || o.turntable == 0)
        throw std::runtime_error("--turntable N[:x|y|z][:M,M,...]: N is a number of projections, at least 1");
    size_t next = 1;
    if (next < parts.size() && (parts[next] == "x" || parts[next] == "y" || parts[next] == "z"))
        o.turn_axis = parts[next++][0] - 'x';
    if (next < parts.size()) {
        for (const std::string& f : split(parts[next++], ',')) {
            unsigned mesh = 0;
            if (!parse_index(f, mesh)) throw std::runtime_error("--turntable: '" + f + "' is not a mesh number");
            o.turn_meshes.push_back(mesh);
        }
    }
    if (next != parts.size()) throw std::runtime_error("--turntable N[:x|y|z][:M,M,...]: '" + arg + "'");
}

// NAME.EXT -> NAME.pKKK.EXT (three digits or more)
std::string projection_name(const std::string& path, unsigned k)
{
    const size_t dot = path.find_last_of("./");
    const bool ext = dot != std::string::npos && path[dot] == '.' && dot > 0 && path[dot - 1] != '/' && path[dot - 1] != '.';
    char num[16];
    std::snprintf(num, sizeof num, ".p%03u", k);
    return ext ? path.substr(0, dot) + num + path.substr(dot) : path + num;
}

unsigned parse_uint(const char* prog, int argc, char** argv, int& i)
{
    if (++i >= argc) {
        showUsage(prog);
        std::exit(EXIT_FAILURE);
    }
    return (unsigned)std::stoi(argv[i]);
}

std::string parse_str(const char* prog, int argc, char** argv, int& i)
{
    if (++i >= argc) {
        showUsage(prog);
        std::exit(EXIT_FAILURE);
    }
    return argv[i];
}

// --spectrum FILE: the first data line is the K weights, every further one a
// mesh's K coefficients ('#' starts a comment, blank lines are skipped).
void read_spectrum(const std::string& path, std::vector<float>& weight, std::vector<float>& mu)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("--spectrum: cannot read " + path);
    std::string line;
    for (unsigned n = 1; std::getline(in, line); ++n) {
        line = line.substr(0, line.find('#'));
        std::istringstream fields(line);
        std::vector<float> row;
        for (std::string f; fields >> f;) {
            size_t used = 0;
            float v = 0.0f;
            try {
                v = std::stof(f, &used);
            } catch (const std::exception&) {
                used = 0;
            }
            if (used != f.size())
                throw std::runtime_error("--spectrum: " + path + ":" + std::to_string(n) + ": '" + f + "' is not a number");
            row.push_back(v);
        }
        if (row.empty()) continue;
        if (weight.empty()) {
            if (row.size() > XRT_MAX_BINS)
                throw std::runtime_error("--spectrum: " + path + ":" + std::to_string(n) + ": " + std::to_string(row.size()) +
                                         " bins, at most " + std::to_string(XRT_MAX_BINS));
            weight = row;
        } else if (row.size() != weight.size()) {
            throw std::runtime_error("--spectrum: " + path + ":" + std::to_string(n) + ": " + std::to_string(row.size()) +
                                     " coefficients in a row, " + std::to_string(weight.size()) + " bins");
        } else {
            mu.insert(mu.end(), row.begin(), row.end());
        }
    }
    if (weight.empty()) throw std::runtime_error("--spectrum: " + path + " holds no weights");
    if (mu.empty()) throw std::runtime_error("--spectrum: " + path + " holds no mesh's coefficients");
}

// A table of rows (--detector FILE, --decompose BASIS): every data line is one
// row of finite values >= 0 ('#' starts a comment, blank lines are skipped), at
// most max_rows of them.  `value` names a value, `row` a row and `many` several
// in the errors.  The lines' length is checked against the spectrum's bins
// once every option is read.
void read_rows(const std::string& option, const std::string& path, const char* value, const char* row, const char* many,
               size_t max_rows, std::vector<std::vector<float>>& rows)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error(option + ": cannot read " + path);
    std::string line;
    for (unsigned n = 1; std::getline(in, line); ++n) {
        line = line.substr(0, line.find('#'));
        std::istringstream fields(line);
        std::vector<float> values;
        for (std::string f; fields >> f;) {
            size_t used = 0;
            float v = 0.0f;
            try {
                v = std::stof(f, &used);
            } catch (const std::exception&) {
                used = 0;
            }
            if (used != f.size() || !std::isfinite(v) || v < 0.0f)
                throw std::runtime_error(option + ": " + path + ":" + std::to_string(n) + ": '" + f + "' is not a " + value +
                                         " (a finite number, >= 0)");
            values.push_back(v);
        }
        if (values.empty()) continue;
        if (rows.size() == max_rows)
            throw std::runtime_error(option + ": " + path + ":" + std::to_string(n) + ": more than " +
                                     std::to_string(max_rows) + " " + many);
        rows.push_back(values);
    }
    if (rows.empty()) throw std::runtime_error(option + ": " + path + " holds no " + row);
}

void check_taps(const std::string& option, const std::string& where, size_t n);

// --scatter FILE: the data lines' fields ('#' starts a comment, blank lines are
// skipped); scatter_model reads them once --spectrum's table is known.
void read_scatter(const std::string& path, std::vector<std::vector<std::string>>& lines)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("--scatter: cannot read " + path);
    lines.clear();
    for (std::string line; std::getline(in, line);) {
        std::istringstream fields(line.substr(0, line.find('#')));
        std::vector<std::string> row;
        for (std::string f; fields >> f;) row.push_back(f);
        if (!row.empty()) lines.push_back(row);
    }
    if (lines.empty()) throw std::runtime_error("--scatter: " + path + " holds no binning factor");
}

// A finite number >= 0 of --scatter's file.
float scatter_value(const std::string& path, const std::string& f, const char* what)
{
    size_t used = 0;
    float v = 0.0f;
    try {
        v = std::stof(f, &used);
    } catch (const std::exception&) {
        used = 0;
    }
    if (f.empty() || used != f.size() || !std::isfinite(v) || v < 0.0f)
        throw std::runtime_error("--scatter: " + path + ": '" + f + "' is not " + what + " (a finite number, >= 0)");
    return v;
}

// --scatter's model from its file's lines under a table of K bins: D, then a
// row of K coefficients per mesh (as many as --spectrum's file holds), then 1
// to XRT_MAX_SCATTER_KERNELS lines AMP SIGMA_PIXELS[:TAPS].
void scatter_model(const std::string& path, const std::vector<std::vector<std::string>>& lines, size_t num_meshes, size_t K,
                   ScatterModel& model)
{
    unsigned D = 0;
    if (lines[0].size() != 1 || !parse_index(lines[0][0], D) || D == 0 || D > XRT_MAX_SCATTER_BIN || (D & (D - 1u)) != 0)
        throw std::runtime_error("--scatter: " + path + ": the first line is the binning factor, a power of two in 1.." +
                                 std::to_string(XRT_MAX_SCATTER_BIN));
    if (lines.size() < 1 + num_meshes + 1 || lines.size() > 1 + num_meshes + XRT_MAX_SCATTER_KERNELS)
        throw std::runtime_error("--scatter: " + path + " holds " + std::to_string(lines.size() - 1) + " lines after the binning factor; " +
                                 std::to_string(num_meshes) + " rows of coefficients (--spectrum's meshes) and 1 to " +
                                 std::to_string(XRT_MAX_SCATTER_KERNELS) + " kernels are expected");
    model = ScatterModel();
    model.bin = D;
    for (size_t m = 0; m < num_meshes; ++m) {
        const std::vector<std::string>& row = lines[1 + m];
        if (row.size() != K)
            throw std::runtime_error("--scatter: " + path + ": " + std::to_string(row.size()) + " coefficients in a line, " +
                                     std::to_string(K) + " bins in --spectrum's table");
        for (const std::string& f : row) model.sigma.push_back(scatter_value(path, f, "a coefficient"));
    }
    for (size_t k = 1 + num_meshes; k < lines.size(); ++k) {
        const std::vector<std::string>& row = lines[k];
        if (row.size() != 2) throw std::runtime_error("--scatter: " + path + ": a kernel line is AMP SIGMA_PIXELS[:TAPS]");
        ScatterKernel kernel;
        kernel.amp = scatter_value(path, row[0], "an amplitude");
        const std::vector<std::string> parts = split(row[1], ':');
        if (parts.empty() || parts.size() > 2) throw std::runtime_error("--scatter: " + path + ": a kernel line is AMP SIGMA_PIXELS[:TAPS]");
        const double sigma = (double)scatter_value(path, parts[0], "a kernel's sigma") / (double)D;
        if (!(sigma > 0.0)) throw std::runtime_error("--scatter: " + path + ": a kernel's SIGMA_PIXELS is above 0");
        unsigned taps = 2u * (unsigned)std::min(std::ceil(4.0 * sigma), 1e6) + 1u;
        if (parts.size() == 2 && !parse_index(parts[1], taps))
            throw std::runtime_error("--scatter: " + path + ": '" + parts[1] + "' is not a tap count");
        check_taps("--scatter", path + ": sigma " + parts[0] + " at D = " + std::to_string(D) + " takes ", taps);
        kernel.taps_x.resize(taps);
        if (xrt_lsf_gaussian(sigma, taps, kernel.taps_x.data()) != XRT_OK)
            throw std::runtime_error("--scatter: " + path + ": '" + row[1] + "' is not a kernel");
        kernel.taps_y = kernel.taps_x;
        model.kernels.push_back(kernel);
    }
}

// --detector FILE: one line of K responses per channel.
void read_detector(const std::string& path, std::vector<std::vector<float>>& rows)
{
    read_rows("--detector", path, "response", "channel", "channels", XRT_MAX_CHANNELS, rows);
}

// --decompose BASIS[:ITER[:TOL]]: BASIS holds one line of K coefficients per
// basis material.
void parse_decompose(const std::string& arg, Options& o)
{
    const std::vector<std::string> parts = split(arg, ':');
    bool ok = parts.size() >= 1 && parts.size() <= 3 && !parts[0].empty();
    if (ok && parts.size() >= 2) ok = parse_index(parts[1], o.decompose_iter) && o.decompose_iter >= 1 && o.decompose_iter <= 200;
    if (ok && parts.size() == 3) {
        size_t used = 0;
        try {
            o.decompose_tol = std::stod(parts[2], &used);
        } catch (const std::exception&) {
            used = 0;
        }
        ok = !parts[2].empty() && used == parts[2].size() && std::isfinite(o.decompose_tol) && o.decompose_tol >= 0.0;
    }
    if (!ok)
        throw std::runtime_error("--decompose BASIS[:ITER[:TOL]]: BASIS a file, ITER iterations (1 to 200), TOL a finite number, >= 0");
    o.basis_rows.clear();
    read_rows("--decompose", parts[0], "coefficient", "basis material", "basis materials", XRT_MAX_BASIS, o.basis_rows);
}

// A channel image as its text file holds it: every value through the writer's
// "%.6g" and back, so that --decompose sees what a reader of the file sees.
void round_as_written(Image& image)
{
    float* v = image.getData();
    char buf[32];
    for (size_t i = 0, n = (size_t)image.getWidth() * image.getHeight(); i < n; ++i) {
        std::snprintf(buf, sizeof buf, "%.6g", (double)v[i]);
        v[i] = (float)std::strtod(buf, nullptr);
    }
}

// --read-noise SIGMA
float parse_read_noise(const std::string& arg)
{
    size_t used = 0;
    float v = 0.0f;
    try {
        v = std::stof(arg, &used);
    } catch (const std::exception&) {
        used = 0;
    }
    if (arg.empty() || used != arg.size() || !std::isfinite(v) || v < 0.0f)
        throw std::runtime_error("--read-noise SIGMA: SIGMA is a finite number of counts, >= 0");
    return v;
}

// A tap count the library takes.
void check_taps(const std::string& option, const std::string& where, size_t n)
{
    if (n % 2 == 0 || n > XRT_MAX_LSF_TAPS)
        throw std::runtime_error(option + ": " + where + std::to_string(n) + " taps; the count must be odd and at most " +
                                 std::to_string(XRT_MAX_LSF_TAPS));
}

// --lsf FILE: the first data line is the taps along x, an optional second one
// those along y ('#' starts a comment, blank lines are skipped).
void read_lsf(const std::string& path, std::vector<float>& lsf_x, std::vector<float>& lsf_y)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("--lsf: cannot read " + path);
    std::string line;
    unsigned rows = 0;
    for (unsigned n = 1; std::getline(in, line); ++n) {
        line = line.substr(0, line.find('#'));
        std::istringstream fields(line);
        std::vector<float> row;
        for (std::string f; fields >> f;) {
            size_t used = 0;
            float v = 0.0f;
            try {
                v = std::stof(f, &used);
            } catch (const std::exception&) {
                used = 0;
            }
            if (used != f.size() || !std::isfinite(v))
                throw std::runtime_error("--lsf: " + path + ":" + std::to_string(n) + ": '" + f + "' is not a finite number");
            row.push_back(v);
        }
        if (row.empty()) continue;
        if (++rows > 2)
            throw std::runtime_error("--lsf: " + path + ":" + std::to_string(n) + ": a third line of taps (x, then y)");
        check_taps("--lsf", path + ":" + std::to_string(n) + ": ", row.size());
        (rows == 1 ? lsf_x : lsf_y) = row;
    }
    if (lsf_x.empty()) throw std::runtime_error("--lsf: " + path + " holds no taps");
    if (lsf_y.empty()) lsf_y = lsf_x;
}

// --lsf-gaussian SIGMA[:TAPS]
void parse_lsf_gaussian(const std::string& arg, std::vector<float>& lsf_x, std::vector<float>& lsf_y)
{
    const std::vector<std::string> parts = split(arg, ':');
    double sigma = 0.0;
    size_t used = 0;
    try {
        sigma = std::stod(parts[0], &used);
    } catch (const std::exception&) {
        used = 0;
    }
    if (parts.size() > 2 || parts[0].empty() || used != parts[0].size() || !std::isfinite(sigma) || !(sigma > 0.0))
        throw std::runtime_error("--lsf-gaussian SIGMA[:TAPS]: SIGMA is a finite number of pixels above 0");
    unsigned taps = (unsigned)std::min(2.0 * std::ceil(4.0 * sigma) + 1.0, (double)XRT_MAX_LSF_TAPS);
    if (parts.size() == 2) {
        if (!parse_index(parts[1], taps)) throw std::runtime_error("--lsf-gaussian SIGMA[:TAPS]: '" + parts[1] + "' is not a tap count");
        check_taps("--lsf-gaussian", "", taps);
    }
    lsf_x.resize(taps);
    if (xrt_lsf_gaussian(sigma, taps, lsf_x.data()) != XRT_OK)
        throw std::runtime_error("--lsf-gaussian SIGMA[:TAPS]: '" + arg + "'");
    lsf_y = lsf_x;
}

// --noise GAIN[:SEED]
void parse_noise(const std::string& arg, Options& o)
{
    const std::vector<std::string> parts = split(arg, ':');
    size_t used = 0;
    try {
        o.noise_gain = std::stof(parts[0], &used);
    } catch (const std::exception&) {
        used = 0;
    }
    if (parts.size() > 2 || parts[0].empty() || used != parts[0].size() || !std::isfinite(o.noise_gain) || !(o.noise_gain > 0.0f))
        throw std::runtime_error("--noise GAIN[:SEED]: GAIN is a finite number of photons per unit of image value, above 0");
    o.noise_seed = 0;
    if (parts.size() == 2) {
        const std::string& s = parts[1];
        used = 0;
        try {
            if (!s.empty() && std::isdigit((unsigned char)s[0])) o.noise_seed = std::stoull(s, &used, 10);
        } catch (const std::exception&) {
            used = 0;
        }
        if (s.empty() || used != s.size())
            throw std::runtime_error("--noise GAIN[:SEED]: '" + s + "' is not a seed (an unsigned 64-bit integer, decimal)");
    }
    o.noise = true;
}

// --focal-spot UxV[:NUxNV]
void parse_focal_spot(const std::string& arg, Options& o)
{
    const std::vector<std::string> parts = split(arg, ':');
    const std::vector<std::string> size = split(parts[0], 'x');
    float v[2] = {0.0f, 0.0f};
    bool ok = parts.size() <= 2 && size.size() == 2;
    for (size_t k = 0; ok && k < 2; ++k) {
        size_t used = 0;
        try {
            v[k] = std::stof(size[k], &used);
        } catch (const std::exception&) {
            used = 0;
        }
        ok = !size[k].empty() && used == size[k].size() && std::isfinite(v[k]) && v[k] >= 0.0f;
    }
    if (!ok)
        throw std::runtime_error("--focal-spot UxV[:NUxNV]: U and V are the spot's sizes in scene units, finite and >= 0");
    o.spot_u = v[0], o.spot_v = v[1];
    o.spot_nu = o.spot_nv = 3;
    if (parts.size() == 2) {
        const std::vector<std::string> grid = split(parts[1], 'x');
        if (grid.size() != 2 || !parse_index(grid[0], o.spot_nu) || !parse_index(grid[1], o.spot_nv) || !o.spot_nu ||
            !o.spot_nv || (unsigned long long)o.spot_nu * o.spot_nv > XRT_MAX_SOURCES)
            throw std::runtime_error("--focal-spot UxV[:NUxNV]: '" + parts[1] + "' is not a grid of 1 to " +
                                     std::to_string(XRT_MAX_SOURCES) + " sub-sources");
    }
    o.focal_spot = true;
}

Options processCmd(int argc, char** argv)
{
    Options o;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "-h" || a == "--help") {
            showUsage(argv[0]);
            std::exit(EXIT_SUCCESS);
        } else if (a == "-s" || a == "--size") {
            o.width = parse_uint(argv[0], argc, argv, i);
            o.height = parse_uint(argv[0], argc, argv, i);
        } else if (a == "-b" || a == "--background") {
            for (int k = 0; k < 3; ++k) (void)parse_uint(argv[0], argc, argv, i);
        } else if (a == "-f" || a == "--filename") {
            o.output = "./out/" + parse_str(argv[0], argc, argv, i);
        } else if (a == "-i" || a == "--input") {
            o.inputs.push_back(parse_str(argv[0], argc, argv, i));
        } else if (a == "-g" || a == "--gpus") {
            o.gpus = (int)parse_uint(argv[0], argc, argv, i);
        } else if (a == "-t" || a == "--threads") {
            (void)parse_uint(argv[0], argc, argv, i);
        } else if (a == "-k" || a == "--kernel") {
            std::string k = parse_str(argv[0], argc, argv, i);
            if (k == "brute") o.kernel = XRT_KERNEL_BRUTE;
            else if (k == "tiled") o.kernel = XRT_KERNEL_TILED;
            else if (k == "binned") o.kernel = XRT_KERNEL_BINNED;
            else {
                showUsage(argv[0]);
                std::exit(EXIT_FAILURE);
            }
        } else if (a == "--lbuffer") {
            o.lbuffer = parse_str(argv[0], argc, argv, i);
        } else if (a == "--u8") {
            o.u8 = parse_str(argv[0], argc, argv, i);
        } else if (a == "--signed") {
            o.signed_model = true;
        } else if (a == "--materials") {
            const std::string list = parse_str(argv[0], argc, argv, i);
            for (size_t pos = 0; pos <= list.size();) {
                size_t next = list.find(',', pos);
                if (next == std::string::npos) next = list.size();
                o.materials.push_back(std::stof(list.substr(pos, next - pos)));
                pos = next + 1;
            }
        } else if (a == "--spectrum") {
            o.spectrum = true;
            read_spectrum(parse_str(argv[0], argc, argv, i), o.spectrum_weight, o.spectrum_mu);
        } else if (a == "--paths") {
            o.paths = true;
        } else if (a == "--pose") {
            parse_pose(parse_str(argv[0], argc, argv, i), o);
        } else if (a == "--turntable") {
            parse_turntable(parse_str(argv[0], argc, argv, i), o);
        } else if (a == "--lsf") {
            o.lsf_file = true;
            read_lsf(parse_str(argv[0], argc, argv, i), o.lsf_x, o.lsf_y);
        } else if (a == "--lsf-gaussian") {
            o.lsf_gauss = true;
            parse_lsf_gaussian(parse_str(argv[0], argc, argv, i), o.lsf_x, o.lsf_y);
        } else if (a == "--log-projection") {
            const std::string f = parse_str(argv[0], argc, argv, i);
            size_t used = 0;
            try {
                o.flat_value = std::stof(f, &used);
            } catch (const std::exception&) {
                used = 0;
            }
            if (f.empty() || used != f.size() || !std::isfinite(o.flat_value) || !(o.flat_value > 0.0f))
                throw std::runtime_error("--log-projection I0: '" + f + "' is not a finite intensity above 0");
            o.log_projection = true;
        } else if (a == "--sinogram") {
            o.sinogram = parse_str(argv[0], argc, argv, i);
        } else if (a == "--reconstruct") {
            const std::vector<std::string> parts = split(parse_str(argv[0], argc, argv, i), ':');
            if (parts.empty() || parts.size() > 2 || parts[0].size() < 5 || parts[0].substr(parts[0].size() - 4) != ".mhd" ||
                (parts.size() == 2 && (!parse_index(parts[1], o.reconstruct_n) || o.reconstruct_n < 1 || o.reconstruct_n > 2048)))
                throw std::runtime_error("--reconstruct FILE.mhd[:N]: a MetaImage header's name and a grid size of 1 to 2048");
            o.reconstruct = parts[0];
        } else if (a == "--voxelize") {
            const std::vector<std::string> parts = split(parse_str(argv[0], argc, argv, i), ':');
            if (parts.empty() || parts.size() > 2 || parts[0].size() < 5 || parts[0].substr(parts[0].size() - 4) != ".mhd" ||
                (parts.size() == 2 && (!parse_index(parts[1], o.voxelize_n) || o.voxelize_n < 1 || o.voxelize_n > 2048)))
                throw std::runtime_error("--voxelize FILE.mhd[:N]: a MetaImage header's name and a grid size of 1 to 2048");
            o.voxelize = parts[0];
        } else if (a == "--sirt") {
            const std::vector<std::string> parts = split(parse_str(argv[0], argc, argv, i), ':');
            bool ok = parts.size() >= 1 && parts.size() <= 3 && parse_index(parts[0], o.sirt_iterations) && o.sirt_iterations >= 1;
            if (ok && parts.size() >= 2)
                ok = parse_index(parts[1], o.sirt_subsets) && o.sirt_subsets >= 1 && o.sirt_subsets <= XRT_MAX_SUBSETS;
            if (ok && parts.size() == 3) {
                size_t used = 0;
                try {
                    o.sirt_relax = std::stod(parts[2], &used);
                } catch (const std::exception&) {
                    used = 0;
                }
                ok = !parts[2].empty() && used == parts[2].size() && std::isfinite(o.sirt_relax);
            }
            if (!ok)
                throw std::runtime_error("--sirt K[:S[:RELAX]]: K iterations (>= 1), S subsets (1 to 64), RELAX a finite number");
        } else if (a == "--mltr") {
            const std::vector<std::string> parts = split(parse_str(argv[0], argc, argv, i), ':');
            bool ok = parts.size() >= 1 && parts.size() <= 3 && parse_index(parts[0], o.mltr_iterations) && o.mltr_iterations >= 1;
            if (ok && parts.size() >= 2)
                ok = parse_index(parts[1], o.mltr_subsets) && o.mltr_subsets >= 1 && o.mltr_subsets <= XRT_MAX_SUBSETS;
            if (ok && parts.size() == 3) {
                size_t used = 0;
                try {
                    o.mltr_relax = std::stod(parts[2], &used);
                } catch (const std::exception&) {
                    used = 0;
                }
                ok = !parts[2].empty() && used == parts[2].size() && std::isfinite(o.mltr_relax);
            }
            if (!ok)
                throw std::runtime_error("--mltr K[:S[:RELAX]]: K iterations (>= 1), S subsets (1 to 64), RELAX a finite number");
        } else if (a == "--tv") {
            const std::vector<std::string> parts = split(parse_str(argv[0], argc, argv, i), ':');
            bool ok = parts.size() >= 1 && parts.size() <= 4 && parse_index(parts[0], o.tv_params.steps) && o.tv_params.steps >= 1;
            double* fields[3] = {&o.tv_params.alpha, &o.tv_params.reduction, &o.tv_params.eps};
            for (size_t f = 1; ok && f < parts.size(); ++f) {
                size_t used = 0;
                try {
                    *fields[f - 1] = std::stod(parts[f], &used);
                } catch (const std::exception&) {
                    used = 0;
                }
                ok = !parts[f].empty() && used == parts[f].size() && std::isfinite(*fields[f - 1]);
            }
            ok = ok && o.tv_params.alpha >= 0.0 && o.tv_params.reduction > 0.0 && o.tv_params.reduction <= 1.0 && o.tv_params.eps > 0.0;
            if (!ok)
                throw std::runtime_error("--tv STEPS[:ALPHA[:REDUCTION[:EPS]]]: STEPS descent steps (>= 1), ALPHA finite and >= 0, REDUCTION in (0, 1], EPS finite and > 0");
            o.tv = true;
        } else if (a == "--noise") {
            parse_noise(parse_str(argv[0], argc, argv, i), o);
        } else if (a == "--supersample") {
            const std::string b = parse_str(argv[0], argc, argv, i);
            if (!parse_index(b, o.supersample) || o.supersample < 1 || o.supersample > XRT_MAX_BIN)
                throw std::runtime_error("--supersample B: '" + b + "' is not a factor in 1.." + std::to_string(XRT_MAX_BIN));
        } else if (a == "--focal-spot") {
            parse_focal_spot(parse_str(argv[0], argc, argv, i), o);
        } else if (a == "--scatter") {
            o.scatter = true;
            o.scatter_file = parse_str(argv[0], argc, argv, i);
            read_scatter(o.scatter_file, o.scatter_lines);
        } else if (a == "--detector") {
            o.detector = true;
            o.detector_rows.clear();
            read_detector(parse_str(argv[0], argc, argv, i), o.detector_rows);
        } else if (a == "--decompose") {
            o.decompose = true;
            parse_decompose(parse_str(argv[0], argc, argv, i), o);
        } else if (a == "--read-noise") {
            o.read_noise = parse_read_noise(parse_str(argv[0], argc, argv, i));
            o.read_noise_set = true;
        } else if (a == "--volume") {
            o.volume = parse_str(argv[0], argc, argv, i);
        } else if (a == "--volume-density") {
            o.volume_density = parse_str(argv[0], argc, argv, i);
        } else if (a == "--time") {
            o.time = true;
        } else if (a == "--rows") {
            const std::string r = parse_str(argv[0], argc, argv, i);
            const size_t colon = r.find(':');
            if (colon == std::string::npos || colon == 0 || colon + 1 >= r.size()) {
                showUsage(argv[0]);
                std::exit(EXIT_FAILURE);
            }
            o.rows = true;
            o.row_begin = (unsigned)std::stoul(r.substr(0, colon));
            o.row_end = (unsigned)std::stoul(r.substr(colon + 1));
        } else if (a == "--batch") {
            o.batch = parse_uint(argv[0], argc, argv, i);
            if (!o.batch) {
                showUsage(argv[0]);
                std::exit(EXIT_FAILURE);
            }
        } else {
            showUsage(argv[0]);
            std::exit(EXIT_FAILURE);
        }
    }
    if (o.inputs.empty() && o.volume.empty()) o.inputs.push_back("./dragon.ply");
    if (o.scatter) {
        if (!o.paths || !o.spectrum) throw std::runtime_error("--scatter needs --paths --spectrum FILE: it reads the planes under the table");
        const char* with = o.detector ? "--detector" : o.supersample ? "--supersample" : o.focal_spot ? "--focal-spot"
                           : !o.volume.empty() ? "--volume" : o.gpus > 1 ? "-g" : o.rows ? "--rows" : o.batch ? "--batch" : nullptr;
        if (with) throw std::runtime_error(std::string("--scatter adds its estimate to whole frames of the meshes' planes on one GPU: not with ") + with);
        scatter_model(o.scatter_file, o.scatter_lines, o.spectrum_mu.size() / o.spectrum_weight.size(), o.spectrum_weight.size(),
                      o.scatter_model);
    }
    if (!o.volume_density.empty() && o.volume.empty())
        throw std::runtime_error("--volume-density needs --volume FILE.mhd: it is the density of that volume's voxels");
    if (!o.volume.empty()) {
        if (!o.paths) throw std::runtime_error("--volume needs --paths: a volume is traced into path-length planes");
        const char* with = o.gpus > 1 ? "-g" : o.rows ? "--rows" : o.batch ? "--batch" : o.supersample ? "--supersample"
                           : o.focal_spot ? "--focal-spot" : o.turntable ? "--turntable" : !o.poses.empty() ? "--pose" : nullptr;
        if (with)
            throw std::runtime_error(std::string("--volume traces whole frames on one GPU and has no pose: not with ") + with);
    }
    if (o.decompose) {
        if (!o.detector) throw std::runtime_error("--decompose needs --detector FILE: it inverts that detector's channels");
        if (o.gpus > 1) throw std::runtime_error("--decompose runs on one GPU: not with -g N");
        for (const std::vector<float>& row : o.basis_rows)
            if (row.size() != o.spectrum_weight.size())
                throw std::runtime_error("--decompose: " + std::to_string(row.size()) + " coefficients in a line, " +
                                         std::to_string(o.spectrum_weight.size()) + " bins in --spectrum's table");
        if (o.basis_rows.size() > o.detector_rows.size())
            throw std::runtime_error("--decompose: " + std::to_string(o.basis_rows.size()) + " basis materials need at least as many channels, --detector's file holds " +
                                     std::to_string(o.detector_rows.size()));
    }
    if (o.rows && (o.row_begin >= o.row_end || o.row_end > o.height))
        throw std::out_of_range("--rows A:B must satisfy 0 <= A < B <= image height");
    if ((o.rows || o.batch) && (o.signed_model || !o.materials.empty() || o.spectrum || o.gpus > 1))
        throw std::runtime_error("--rows and --batch render the attenuation model on one GPU");
    if (o.paths && (o.signed_model || !o.materials.empty()))
        throw std::runtime_error("--paths, --signed and --materials are three models: give one");
    if (o.paths && (o.rows || o.batch || o.gpus > 1))
        throw std::runtime_error("--paths renders whole frames on one GPU");
    if (o.detector) {                           // (the channels do not go through the rest of the chain yet)
        if (!o.paths || !o.spectrum) throw std::runtime_error("--detector needs --paths --spectrum FILE: it reads the planes under the table");
        if (!o.lsf_x.empty() || o.log_projection || !o.sinogram.empty() || o.supersample || o.focal_spot || o.gpus > 1 ||
            o.rows || o.batch)
            throw std::runtime_error("--detector writes its channels as detected: not with --lsf, --lsf-gaussian, "
                                     "--log-projection, --sinogram, --supersample, --focal-spot, -g N, --rows or --batch");
        for (const std::vector<float>& row : o.detector_rows)
            if (row.size() != o.spectrum_weight.size())
                throw std::runtime_error("--detector: " + std::to_string(row.size()) + " responses in a line, " +
                                         std::to_string(o.spectrum_weight.size()) + " bins in --spectrum's table");
    }
    if (o.read_noise_set && (!o.detector || !o.noise))
        throw std::runtime_error("--read-noise needs --detector FILE and --noise GAIN[:SEED]: it is added to the drawn channels");
    if (o.turntable && ((o.paths && !o.detector && !o.scatter) || o.batch || o.gpus > 1))
        throw std::runtime_error("--turntable renders on one GPU, without --paths, --batch and -g");
    if (o.lsf_file && o.lsf_gauss) throw std::runtime_error("--lsf and --lsf-gaussian are two detector responses: give one");
    if (!o.lsf_x.empty() && (o.gpus > 1 || o.rows))
        throw std::runtime_error(std::string(o.lsf_file ? "--lsf" : "--lsf-gaussian") +
                                 " needs whole frames on one GPU: not with -g N or --rows");
    if (!o.lsf_x.empty() && o.paths && !o.spectrum)
        throw std::runtime_error(std::string(o.lsf_file ? "--lsf" : "--lsf-gaussian") +
                                 " with --paths needs --spectrum: the planes stay as rendered, there is no image to spread");
    if (!o.sinogram.empty() && (!o.turntable || !o.log_projection))
        throw std::runtime_error("--sinogram needs --turntable N and --log-projection I0: it stacks a scan's line integrals");
    if (!o.reconstruct.empty() && (!o.turntable || !o.log_projection))
        throw std::runtime_error("--reconstruct needs --turntable N and --log-projection I0: it reconstructs a scan's line integrals");
    if (!o.reconstruct.empty() && !o.turn_meshes.empty())
        throw std::runtime_error("--reconstruct needs a --turntable that turns every mesh: the scene is reconstructed as one object");
    if (o.sirt_iterations && o.reconstruct.empty())
        throw std::runtime_error("--sirt needs --reconstruct FILE.mhd: it chooses how the scan is reconstructed");
    if (o.mltr_iterations && o.sirt_iterations)
        throw std::runtime_error("--mltr and --sirt are two solvers: give one");
    if (o.mltr_iterations && o.reconstruct.empty())
        throw std::runtime_error("--mltr needs --reconstruct FILE.mhd: it chooses how the scan is reconstructed");
    if (o.tv && !o.sirt_iterations && !o.mltr_iterations)
        throw std::runtime_error("--tv needs --sirt K or --mltr K: it regularises the iterative reconstruction");
    if (o.mltr_iterations && o.mltr_subsets > o.turntable)
        throw std::runtime_error("--mltr K[:S[:RELAX]]: more subsets than projections");
    if (o.sirt_iterations && o.sirt_subsets > o.turntable)
        throw std::runtime_error("--sirt K[:S[:RELAX]]: more subsets than projections");
    if (o.log_projection && (o.gpus > 1 || o.rows))
        throw std::runtime_error("--log-projection needs whole frames on one GPU: not with -g N or --rows");
    if (o.log_projection && o.paths && !o.spectrum)
        throw std::runtime_error("--log-projection with --paths needs --spectrum: the planes stay as rendered, there is no image");
    if (o.noise && (o.gpus > 1 || o.rows))
        throw std::runtime_error("--noise needs whole frames on one GPU: not with -g N or --rows");
    if (o.noise && o.paths && !o.spectrum)
        throw std::runtime_error("--noise with --paths needs --spectrum: the planes stay as rendered, there is no image");
    if (o.supersample || o.focal_spot) {
        const std::string which = o.supersample ? "--supersample" : "--focal-spot";
        if (o.gpus > 1 || o.rows || o.batch || o.paths)
            throw std::runtime_error(which + " integrates whole frames on one GPU: not with -g N, --rows, --batch or --paths");
        if (!o.lbuffer.empty())
            throw std::runtime_error(which + " with --lbuffer: an integrated frame has no single L-buffer");
        if ((unsigned long long)o.width * std::max(o.supersample, 1u) > 0x7FFFFFFFull ||
            (unsigned long long)o.height * std::max(o.supersample, 1u) > 0x7FFFFFFFull)
            throw std::runtime_error(which + ": the supersampled frame is above 2^31 - 1 pixels a side");
    }
    if (o.signed_model && !o.materials.empty())
        throw std::runtime_error("--signed and --materials are two models: give one");
    if (o.spectrum && (o.signed_model || !o.materials.empty()))
        throw std::runtime_error("--spectrum, --signed and --materials are three models: give one");
    return o;
}

// The grid of --reconstruct and --voxelize, so that truth and reconstruction share voxels: n^3 voxels, a cube
// about the box centre of the scene as loaded -- the turntable's centre -- whose side is the box's diagonal, so
// that it holds the scene under every turn.
void scan_grid(const Vec3& lower, const Vec3& upper, unsigned n, unsigned dims[3], float centre[3], float origin[3],
               float spacing[3])
{
    double diagonal = 0.0;
    for (unsigned k = 0; k < 3; ++k) diagonal += (double)(upper[k] - lower[k]) * (double)(upper[k] - lower[k]);
    diagonal = std::sqrt(diagonal);
    for (unsigned k = 0; k < 3; ++k) {
        dims[k] = n;
        centre[k] = lower[k] + (float)((double)(upper[k] - lower[k]) / 2.0);
        spacing[k] = (float)(diagonal / n);
        origin[k] = (float)((double)centre[k] - diagonal / 2.0);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    try {
        Options opt = processCmd(argc, argv);
        setRenderKernel(opt.kernel);

        std::cout << "Loading polygon meshes... " << std::endl;
        auto t0 = std::chrono::high_resolution_clock::now();
        std::vector<TriangleMesh> meshes;
        if (!opt.inputs.empty()) loadMeshes(opt.inputs[0], meshes);
        for (size_t f = 1; f < opt.inputs.size(); ++f) appendMeshes(opt.inputs[f], meshes);
        Volume volume;                                // --volume: every check before a device is opened
        if (!opt.volume.empty()) {
            try {
                loadVolume(opt.volume, volume);
            } catch (const VolumeError& e) {
                throw std::runtime_error(std::string("--volume: ") + e.what());
            }
            try {
                if (!opt.volume_density.empty()) loadVolumeDensity(opt.volume_density, volume);
            } catch (const VolumeError& e) {
                throw std::runtime_error(std::string("--volume-density: ") + e.what());
            }
            if (volume.num_labels == 0) throw std::runtime_error("--volume: " + opt.volume + " holds no label above 0");
            if (meshes.size() + volume.num_labels > XRT_MAX_MESHES)
                throw std::runtime_error("--volume: " + std::to_string(meshes.size()) + " meshes and " +
                                         std::to_string(volume.num_labels) + " labels are more than " +
                                         std::to_string(XRT_MAX_MESHES) + " planes");
            if (opt.spectrum && opt.spectrum_mu.size() / opt.spectrum_weight.size() != meshes.size() + volume.num_labels)
                throw std::runtime_error("--spectrum takes one row of coefficients per mesh, then one per label of --volume: " +
                                         std::to_string(meshes.size()) + " meshes and " + std::to_string(volume.num_labels) +
                                         " labels loaded, " +
                                         std::to_string(opt.spectrum_mu.size() / opt.spectrum_weight.size()) + " rows");
        }
        auto t1 = std::chrono::high_resolution_clock::now();
        std::cout << "Loading meshes took: " << std::chrono::duration<double>(t1 - t0).count()
                  << " seconds" << std::endl
                  << std::endl;

        for (const auto& q : opt.poses)
            if (q.first >= meshes.size())
                throw std::runtime_error("--pose: mesh " + std::to_string(q.first) + " is not a mesh of the scene (" +
                                         std::to_string(meshes.size()) + " meshes loaded)");
        for (unsigned m : opt.turn_meshes)
            if (m >= meshes.size())
                throw std::runtime_error("--turntable: mesh " + std::to_string(m) + " is not a mesh of the scene (" +
                                         std::to_string(meshes.size()) + " meshes loaded)");

        std::cout << "Getting scene bbox... " << std::endl;
        Vec3 lower, upper;
        getBBox(meshes, upper, lower);
        if (!opt.volume.empty()) {                    // the union of the scene's box and the volume's
            Vec3 vlower, vupper;
            getVolumeBBox(volume, vupper, vlower);
            for (unsigned k = 0; k < 3; ++k) {
                lower[k] = std::min(lower[k], vlower[k]);
                upper[k] = std::max(upper[k], vupper[k]);
            }
        }
        float lut = 0.0f;
        Image image(opt.width, opt.height, lut);
        RayTracerInfo info = initialiseRayTracing(meshes, upper, lower, opt.height, opt.width, image, lut);

        if (!opt.reconstruct.empty()) {               // before a projection is rendered: the scan is of no use otherwise
            float axis[3] = {0.0f, 0.0f, 0.0f};
            axis[opt.turn_axis] = 1.0f;
            const Vec3 turn_axis(axis[0], axis[1], axis[2]);
            if (std::fabs(turn_axis.dotProduct(info.right)) > 1e-6f * info.right.getLength() ||
                std::fabs(turn_axis.dotProduct(info.detector_position - info.origin)) >
                    1e-6f * (info.detector_position - info.origin).getLength())
                throw std::runtime_error("--reconstruct: the turntable's axis must be parallel to the detector's up, --turntable N:z "
                                         "(the filter runs along the detector's rows)");
        }

        // the poses: --pose's, and over them each projection's turn of --turntable's meshes
        const std::array<float, 12> rest = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
        std::vector<std::array<float, 12>> poses;
        if (!opt.poses.empty() || opt.turntable) poses.assign(meshes.size(), rest);
        for (const auto& q : opt.poses) poses[q.first] = q.second;
        if (!opt.voxelize.empty()) {                  // the scene as --pose leaves it, the turntable's meshes at rest
            if (meshes.empty()) throw std::runtime_error("--voxelize needs a scene: give -i");
            if (!opt.materials.empty() && opt.materials.size() != meshes.size())
                throw std::runtime_error("--materials takes one coefficient per mesh: " + std::to_string(meshes.size()) +
                                         " meshes loaded, " + std::to_string(opt.materials.size()) + " coefficients given");
            float centre[3], origin[3], spacing[3];
            unsigned dims[3];
            scan_grid(lower, upper, opt.voxelize_n, dims, centre, origin, spacing);
            setMeshPoses(opt.poses.empty() ? std::vector<std::array<float, 12>>() : poses);
            Volume truth;
            std::vector<float> mu;
            const unsigned long long odd =
                voxelizeScene(truth, meshes, dims, origin, spacing, opt.materials, opt.materials.empty() ? nullptr : &mu);
            if (odd) std::cout << "--voxelize: " << odd << " grid columns cross an open mesh" << std::endl;
            try {
                saveVolume(opt.voxelize, dims, origin, spacing, truth.labels.data());
                if (!opt.materials.empty())
                    saveVolume(opt.voxelize.substr(0, opt.voxelize.size() - 4) + ".mu.mhd", dims, origin, spacing, mu.data());
            } catch (const VolumeError& e) {
                throw std::runtime_error(std::string("--voxelize: ") + e.what());
            }
        }
        const std::string name = opt.output, lbuffer_name = opt.lbuffer, u8_name = opt.u8;
        std::vector<float> scan;                      // --sinogram: the projections' intensity images
        std::vector<float> integrals;                 // --reconstruct: the projections' line integrals
        std::vector<float> counts, backgrounds;       // --mltr: their intensities before the logarithm, --scatter's estimates
        std::vector<std::array<float, 12>> turns;     //                and the turntable's pose under each
        for (unsigned projection = 0; projection < std::max(opt.turntable, 1u); ++projection) {
            if (opt.turntable) {
                // the rest scene's box centre, as initialiseRayTracing forms it (main.cxx:575-578)
                float axis[3] = {0.0f, 0.0f, 0.0f}, centre[3];
                axis[opt.turn_axis] = 1.0f;
                for (unsigned k = 0; k < 3; ++k) centre[k] = lower[k] + (float)((double)(upper[k] - lower[k]) / 2.0);
                std::array<float, 12> turn;
                if (xrt_pose_rotation(axis, projection * 360.0 / opt.turntable, centre, turn.data()) != XRT_OK)
                    throw std::runtime_error("--turntable: the scene's box is not finite");
                if (!opt.reconstruct.empty()) turns.push_back(turn);
                for (size_t m = 0; m < meshes.size(); ++m)
                    if (opt.turn_meshes.empty() ||
                        std::find(opt.turn_meshes.begin(), opt.turn_meshes.end(), (unsigned)m) != opt.turn_meshes.end())
                        poses[m] = turn;
                opt.output = projection_name(name, projection);
                if (!lbuffer_name.empty()) opt.lbuffer = projection_name(lbuffer_name, projection);
                if (!u8_name.empty()) opt.u8 = projection_name(u8_name, projection);
            }
            setMeshPoses(poses);

            auto r0 = std::chrono::high_resolution_clock::now();
            std::vector<float> lb;
            const unsigned rb = opt.rows ? opt.row_begin : 0u, re = opt.rows ? opt.row_end : opt.height;
            double ms_per_frame = 0.0;
            const bool area = opt.supersample || opt.focal_spot;
            const unsigned bin = std::max(opt.supersample, 1u);
            // the model's whole-frame render of `img` (its size) as seen from `inf`
            const auto render_model = [&](Image& img, RayTracerInfo& inf) {
                if (!opt.materials.empty()) {
                    if (opt.materials.size() != meshes.size())
                        throw std::runtime_error("--materials takes one coefficient per mesh: " + std::to_string(meshes.size()) +
                                                 " meshes loaded, " + std::to_string(opt.materials.size()) + " coefficients");
                    std::vector<float>* l = opt.lbuffer.empty() ? nullptr : &lb;
                    if (opt.gpus > 1) renderLoopMaterialsMultiGPU(img, meshes, inf, opt.materials, opt.gpus, l);
                    else renderLoopMaterials(img, meshes, inf, opt.materials, l);
                } else if (opt.spectrum) {
                    const size_t rows = opt.spectrum_mu.size() / opt.spectrum_weight.size();
                    if (rows != meshes.size())
                        throw std::runtime_error("--spectrum takes one row of coefficients per mesh: " + std::to_string(meshes.size()) +
                                                 " meshes loaded, " + std::to_string(rows) + " rows");
                    std::vector<float>* l = opt.lbuffer.empty() ? nullptr : &lb;
                    if (opt.gpus > 1)
                        renderLoopSpectrumMultiGPU(img, meshes, inf, opt.spectrum_weight, opt.spectrum_mu, opt.gpus, l);
                    else renderLoopSpectrum(img, meshes, inf, opt.spectrum_weight, opt.spectrum_mu, l);
                } else if (opt.signed_model && opt.gpus > 1) {
                    renderLoopLBufferMultiGPU(img, meshes, inf, opt.gpus, opt.lbuffer.empty() ? nullptr : &lb);
                } else if (opt.signed_model) {
                    renderLoopLBuffer(img, meshes, inf, opt.lbuffer.empty() ? nullptr : &lb);
                } else if (opt.gpus > 1) {
                    renderLoopMultiGPU(img, meshes, inf, opt.gpus);
                } else if (!opt.lbuffer.empty()) {       // the image and the L-buffer in one render
                    lb.resize((size_t)img.getWidth() * (re - rb));
                    xrt_stats st;
                    renderLoopRows(img, meshes, inf, rb, re, lb.data(), nullptr, &st);
                    for (unsigned long long k = 0; k < st.odd_rays; ++k) std::cout << "Only one intersect on this ray" << std::endl;
                } else {
                    renderLoop(img, meshes, inf);
                }
            };
            if (opt.batch) {                          // N frames back to back, the last one kept
                xrt_stats st;
                ms_per_frame = renderLoopFrames(image, meshes, info, opt.batch, rb, re, &st);
                for (unsigned long long k = 0; k < st.odd_rays; ++k) std::cout << "Only one intersect on this ray" << std::endl;
            } else if (opt.rows && opt.lbuffer.empty()) {
                xrt_stats st;
                renderLoopRows(image, meshes, info, rb, re, nullptr, nullptr, &st);
                for (unsigned long long k = 0; k < st.odd_rays; ++k) std::cout << "Only one intersect on this ray" << std::endl;
            } else if (opt.paths) {
                const bool with_volume = !opt.volume.empty();
                if (opt.scatter && opt.scatter_model.sigma.size() / opt.spectrum_weight.size() != meshes.size())
                    throw std::runtime_error("--scatter takes one row of coefficients per mesh, as --spectrum does: " +
                                             std::to_string(meshes.size()) + " meshes loaded, " +
                                             std::to_string(opt.scatter_model.sigma.size() / opt.spectrum_weight.size()) + " rows");
                if (!with_volume && opt.spectrum && opt.spectrum_mu.size() / opt.spectrum_weight.size() != meshes.size())
                    throw std::runtime_error("--spectrum takes one row of coefficients per mesh: " + std::to_string(meshes.size()) +
                                             " meshes loaded, " +
                                             std::to_string(opt.spectrum_mu.size() / opt.spectrum_weight.size()) + " rows");
                std::vector<std::vector<float>> planes;
                std::vector<unsigned short> open;
                if (!with_volume) {
                    renderLoopPaths(planes, open, image, meshes, info);
                } else {                              // the meshes' planes (if any), then the labels', under one camera
                    if (!meshes.empty()) renderLoopPaths(planes, open, image, meshes, info, true);
                    else open.assign((size_t)opt.width * opt.height, 0);
                    std::vector<std::vector<float>> labels;
                    uploadVolume(volume);
                    renderLoopVolumePaths(labels, image, info);
                    planes.insert(planes.end(), labels.begin(), labels.end());
                }
                const size_t dot = opt.output.find_last_of("./");
                const bool ext = dot != std::string::npos && opt.output[dot] == '.';
                const std::string stem = ext ? opt.output.substr(0, dot) : opt.output;
                const std::string suffix = ext ? opt.output.substr(dot) : "";
                Image plane(opt.width, opt.height, 0.0f);
                for (size_t m = 0; m < planes.size(); ++m) {
                    std::copy(planes[m].begin(), planes[m].end(), plane.getData());
                    plane.saveTextFile(stem + ".m" + std::to_string(m) + suffix);
                }
                std::copy(open.begin(), open.end(), plane.getData());
                plane.saveTextFile(stem + ".open" + suffix);
                if (opt.scatter) {                    // the primary and the estimate in one pass; the image is their sum
                    Image scattered(opt.width, opt.height, 0.0f);
                    applyScatter(image, scattered, planes, open, opt.spectrum_weight, opt.spectrum_mu, opt.scatter_model,
                                 opt.lbuffer.empty() ? nullptr : &lb);
                    scattered.saveTextFile(stem + ".scatter" + suffix);
                    if (opt.mltr_iterations)          // the estimate is the solver's background
                        backgrounds.insert(backgrounds.end(), scattered.getData(),
                                           scattered.getData() + (size_t)opt.width * opt.height);
                } else if (opt.spectrum)              // (without a table the planes are the output)
                    applySpectrum(image, planes, open, opt.spectrum_weight, opt.spectrum_mu, opt.lbuffer.empty() ? nullptr : &lb);
                if (opt.detector) {                   // the channels beside the image; a scan's projection draws its own
                    std::vector<float> response;
                    for (const std::vector<float>& row : opt.detector_rows) response.insert(response.end(), row.begin(), row.end());
                    std::vector<Image> channels(opt.detector_rows.size(), Image(opt.width, opt.height, 0.0f));
                    applySpectralDetector(channels, planes, open, opt.spectrum_weight, opt.spectrum_mu, response,
                                          opt.noise ? opt.noise_gain : 1.0f, opt.noise ? opt.read_noise : 0.0f,
                                          opt.noise_seed, (unsigned long long)projection * opt.width * opt.height, opt.noise);
                    for (size_t c = 0; c < channels.size(); ++c)
                        channels[c].saveTextFile(stem + ".c" + std::to_string(c) + suffix);
                    if (opt.decompose) {              // the channels as the files hold them, into one plane per basis material
                        for (Image& channel : channels) round_as_written(channel);
                        std::vector<float> basis_mu;
                        for (const std::vector<float>& row : opt.basis_rows) basis_mu.insert(basis_mu.end(), row.begin(), row.end());
                        std::vector<Image> basis(opt.basis_rows.size(), Image(opt.width, opt.height, 0.0f));
                        const unsigned long long unconverged =
                            decomposeMaterials(basis, channels, opt.spectrum_weight, basis_mu, response,
                                               opt.noise ? opt.noise_gain : 1.0f, opt.decompose_iter, opt.decompose_tol);
                        for (size_t b = 0; b < basis.size(); ++b)
                            basis[b].saveTextFile(stem + ".b" + std::to_string(b) + suffix);
                        std::cout << "Decomposition: " << unconverged << " of " << (size_t)opt.width * opt.height
                                  << " pixels failed or ran " << opt.decompose_iter << " iterations" << std::endl;
                    }
                }
            } else if (area) {                        // every sub-source at the finer size, then one integration
                std::vector<RayTracerInfo> sources(1, info);
                if (opt.focal_spot) sources = focalSpotSources(info, opt.spot_u, opt.spot_v, opt.spot_nu, opt.spot_nv);
                std::vector<Image> samples;
                for (RayTracerInfo& source : sources) {
                    samples.emplace_back(opt.width * bin, opt.height * bin, lut);
                    render_model(samples.back(), source);
                }
                applyAreaIntegration(image, samples, bin, bin, std::vector<float>(samples.size(), 1.0f));
            } else {
                render_model(image, info);
            }
            auto r1 = std::chrono::high_resolution_clock::now();
            if (opt.time) {
                double s = std::chrono::duration<double>(r1 - r0).count();
                const double rays = (double)opt.width * (re - rb);
                std::cout << "Render took: " << s << " seconds (" << rays * (opt.batch ? opt.batch : 1) / s / 1e6
                          << " Mrays/s, " << opt.gpus << " GPU(s))" << std::endl;
                if (opt.batch)
                    std::cout << "Frames: " << opt.batch << ", device time per frame " << ms_per_frame << " ms ("
                              << rays / (ms_per_frame * 1e3) << " Mrays/s)" << std::endl;
            }

            // the detector's response, over the image only (the L-buffer and the planes stay as rendered)
            if (!opt.lsf_x.empty()) applyDetectorResponse(image, opt.lsf_x, opt.lsf_y);

            Image* out = &image;
            Image strip;
            if (opt.rows) {                           // the strip's rows only
                strip = Image(opt.width, re - rb, 0.0f);
                std::copy(image.getData() + (size_t)rb * opt.width, image.getData() + (size_t)re * opt.width,
                          strip.getData());
                out = &strip;
            }
            if (opt.paths && !opt.spectrum) return 0;
            if (opt.log_projection || (opt.noise && !opt.detector)) {    // (whole frames: out is the image)
                // the 8-bit image is the rendered intensity's (the 0..80 window means nothing for line integrals)
                if (!opt.u8.empty()) image.savePGMFile(opt.u8, 0.0f, 80.0f);
                Image written(image);
                if (opt.noise)                        // a scan's projection draws what it would draw in the stack
                    applyPhotonNoise(written, opt.noise_gain, opt.noise_seed,
                                     (unsigned long long)projection * opt.width * opt.height);
                if (!opt.sinogram.empty()) scan.insert(scan.end(), written.getData(), written.getData() + (size_t)opt.width * opt.height);
                if (opt.mltr_iterations)              // the intensity as it stands just before the logarithm
                    counts.insert(counts.end(), written.getData(), written.getData() + (size_t)opt.width * opt.height);
                if (opt.log_projection) applyLogProjection(written, opt.flat_value);
                if (!opt.reconstruct.empty())
                    integrals.insert(integrals.end(), written.getData(), written.getData() + (size_t)opt.width * opt.height);
                written.saveTextFile(opt.output);
            } else {
                out->saveTextFile(opt.output);
                if (!opt.u8.empty()) out->savePGMFile(opt.u8, 0.0f, 80.0f);
            }
            if (!opt.lbuffer.empty()) {
                if (lb.empty()) {                   // multi-GPU, batch: the L-buffer of the same frame
                    lb.resize((size_t)opt.width * (re - rb));
                    xrt_stats st;
                    renderLoopRows(image, meshes, info, rb, re, lb.data(), nullptr, &st);
                }
                std::FILE* f = std::fopen(opt.lbuffer.c_str(), "wb");
                if (!f) throw std::runtime_error("Cannot create the file " + opt.lbuffer);
                std::fwrite(lb.data(), sizeof(float), lb.size(), f);
                std::fclose(f);
            }
        }
        if (!opt.sinogram.empty()) {                  // the scan in one call, one sinogram per detector row
            std::vector<float> sinograms;
            logProjectionSinograms(scan, opt.width, opt.height, opt.turntable, opt.flat_value, 0.0f, sinograms);
            std::FILE* f = std::fopen(opt.sinogram.c_str(), "wb");
            if (!f) throw std::runtime_error("Cannot create the file " + opt.sinogram);
            std::fwrite(sinograms.data(), sizeof(float), sinograms.size(), f);
            std::fclose(f);
        }
        if (!opt.reconstruct.empty()) {
            float centre[3], origin[3], spacing[3];
            unsigned dims[3];
            scan_grid(lower, upper, opt.reconstruct_n, dims, centre, origin, spacing);
            std::vector<float> reconstruction;
            if (opt.mltr_iterations) {
                // the planes the solver receives, kept beside the volume: FILE.counts.mhd (and FILE.background.mhd)
                const std::string stem = opt.reconstruct.substr(0, opt.reconstruct.size() - 4);
                const unsigned stack[3] = {opt.width, opt.height, opt.turntable};
                const float zero[3] = {0.0f, 0.0f, 0.0f}, one[3] = {1.0f, 1.0f, 1.0f};
                try {
                    saveVolume(stem + ".counts.mhd", stack, zero, one, counts.data());
                    if (!backgrounds.empty()) saveVolume(stem + ".background.mhd", stack, zero, one, backgrounds.data());
                } catch (const VolumeError& e) {
                    throw std::runtime_error(std::string("--mltr: ") + e.what());
                }
                reconstructMLTR(reconstruction, counts, std::vector<float>((size_t)opt.width * opt.height, opt.flat_value),
                                backgrounds, opt.turntable, image, meshes, info, turns, dims, origin, spacing,
                                opt.mltr_iterations, opt.mltr_subsets, opt.mltr_relax, 0.0f,
                                std::numeric_limits<float>::infinity(), opt.tv ? opt.tv_params : TVParams());
            } else if (opt.sirt_iterations)
                reconstructSIRT(reconstruction, integrals, opt.turntable, image, meshes, info, turns, dims, origin, spacing,
                                opt.sirt_iterations, opt.sirt_subsets, opt.sirt_relax, 0.0f,
                                std::numeric_limits<float>::infinity(), opt.tv ? opt.tv_params : TVParams());
            else
                reconstructFDK(reconstruction, integrals, opt.turntable, image, meshes, info, turns, dims, origin, spacing, centre);
            try {
                saveVolume(opt.reconstruct, dims, origin, spacing, reconstruction.data());
            } catch (const VolumeError& e) {
                throw std::runtime_error(std::string("--reconstruct: ") + e.what());
            }
        }
    } catch (const std::exception& e) {
        std::cerr << "ERROR: " << e.what() << std::endl;
        return 1;
    } catch (const std::string& e) {
        std::cerr << "ERROR: " << e << std::endl;
        return 2;
    } catch (const char* e) {
        std::cerr << "ERROR: " << e << std::endl;
        return 3;
    }
    return 0;
}
