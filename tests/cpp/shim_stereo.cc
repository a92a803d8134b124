// stereo::Stereo (include/aerial-mapper-dense-pcl/stereo.h) driven like main-dense-pcl.cc and
// main-ortho-backward-grid-incremental.cc drive the reference's class, on a sequence the Python test
// wrote to a binary file together with the clouds it expects (tests/stereo_sequence.py's CPU chain):
//   int64  F, W, H, nth, use_bm, n_seq, n_last
//   double fu, fv, cu, cv, T_C_B[7], T_G_B[F][7]
//   uint8  frames[F][H][W]
//   double xyz_seq[n_seq][3];  int32 inten_seq[n_seq]      (addFrames over all frames)
//   double xyz_last[n_last][3]; int32 inten_last[n_last]   (the last pair of the selected frames)
// Exit status 0 = every comparison bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "aerial-mapper-dense-pcl/stereo.h"

typedef AlignedType<std::vector, Eigen::Vector3d>::type Cloud;

template <typename T>
static bool read_n(std::FILE* f, std::vector<T>* out, size_t n) {
  out->resize(n);
  return n == 0 || std::fread(out->data(), sizeof(T), n, f) == n;
}

static int compare(const char* what, const Cloud& cloud, const std::vector<int>& inten,
                   const std::vector<double>& xyz, const std::vector<int32_t>& want_i) {
  if (cloud.size() * 3 != xyz.size() || inten.size() != want_i.size()) {
    std::printf("%s: %zu points (%zu intensities), expected %zu\n", what, cloud.size(), inten.size(),
                want_i.size());
    return 1;
  }
  for (size_t k = 0; k < cloud.size(); ++k)
    if (std::memcmp(cloud[k].data(), &xyz[3 * k], 3 * sizeof(double)) != 0 || inten[k] != want_i[k]) {
      std::printf("%s: point %zu differs\n", what, k);
      return 1;
    }
  std::printf("%s: %zu points ok\n", what, cloud.size());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t h[7];
  if (std::fread(h, sizeof(int64_t), 7, f) != 7) return 2;
  const size_t F = h[0], W = h[1], H = h[2], nth = h[3], n_seq = h[5], n_last = h[6];
  const bool use_bm = h[4] != 0;
  std::vector<double> cam, tgb, xyz_seq, xyz_last;
  std::vector<uint8_t> frames;
  std::vector<int32_t> i_seq, i_last;
  if (!read_n(f, &cam, 11) || !read_n(f, &tgb, 7 * F) || !read_n(f, &frames, F * W * H) ||
      !read_n(f, &xyz_seq, 3 * n_seq) || !read_n(f, &i_seq, n_seq) ||
      !read_n(f, &xyz_last, 3 * n_last) || !read_n(f, &i_last, n_last))
    return 2;
  std::fclose(f);

  const aslam::Camera camera(cam[0], cam[1], cam[2], cam[3], static_cast<uint32_t>(W),
                             static_cast<uint32_t>(H));
  const aslam::Transformation T_C_B(kindr::minimal::RotationQuaternion(cam[7], cam[8], cam[9], cam[10]),
                                    Eigen::Vector3d(cam[4], cam[5], cam[6]));
  std::shared_ptr<aslam::NCamera> ncameras(new aslam::NCamera(camera, T_C_B));
  stereo::Poses poses;
  stereo::Images images;
  for (size_t k = 0; k < F; ++k) {
    const double* p = &tgb[7 * k];
    poses.push_back(stereo::Pose(kindr::minimal::RotationQuaternion(p[3], p[4], p[5], p[6]),
                                 Eigen::Vector3d(p[0], p[1], p[2])));
    images.push_back(cv::Mat(static_cast<int>(H), static_cast<int>(W), 1, &frames[k * W * H], W));
  }
  stereo::Settings settings;
  settings.use_every_nth_image = nth;
  settings.show_rectification = false;
  stereo::BlockMatchingParameters bmp;
  bmp.use_BM = use_bm;
  int bad = 0;
  {
    stereo::Stereo stereo(ncameras, settings, bmp);
    Cloud cloud(3, Eigen::Vector3d(1.0, 2.0, 3.0));   // addFrames clears what it is handed
    std::vector<int> inten(5, 7);
    stereo.addFrames(poses, images, &cloud, &inten);
    bad += compare("addFrames", cloud, inten, xyz_seq, i_seq);
    Cloud only;                                        // the intensities are optional
    stereo::Stereo again(ncameras, settings, bmp);
    again.addFrames(poses, images, &only);
    bad += only.size() == n_seq ? 0 : 1;
    if (stereo.pointCloud2Payload().size() != W * H * 16) ++bad;
  }
  {
    // frame by frame, the way main-ortho-backward-grid-incremental.cc:149 does: every call after
    // the first REPLACES the cloud with that pair's; the first leaves it untouched
    stereo::Stereo stereo(ncameras, settings, bmp);
    Cloud cloud(2, Eigen::Vector3d(4.0, 5.0, 6.0));
    std::vector<int> inten(2, 9);
    size_t used = 0;
    for (size_t k = 0; k < F; ++k) {
      if ((k + 1) % nth != 0) continue;
      stereo.addFrame(poses[k], images[k], &cloud, &inten);
      if (used++ == 0 && (cloud.size() != 2 || cloud[1](2) != 6.0 || inten.size() != 2)) {
        std::printf("addFrame: the first call touched the caller's cloud\n");
        ++bad;
      }
    }
    bad += compare("addFrame (last pair)", cloud, inten, xyz_last, i_last);
  }
  std::printf(bad ? "FAILED\n" : "OK\n");
  return bad ? 1 : 0;
}
