// stereo::Stereo::setPairsInFlight (include/aerial-mapper-dense-pcl/stereo.h): the cloud of an object
// that keeps three pairs in flight is, bit for bit, the cloud of a default object.  The sequence file
// is the one tests/cpp/shim_stereo.cc reads (its expected clouds are read past: both objects here
// are also held to them).
//   int64  F, W, H, nth, use_bm, n_seq, n_last
//   double fu, fv, cu, cv, T_C_B[7], T_G_B[F][7]
//   uint8  frames[F][H][W]
//   double xyz_seq[n_seq][3];  int32 inten_seq[n_seq]
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
  const size_t F = h[0], W = h[1], H = h[2], nth = h[3], n_seq = h[5];
  const bool use_bm = h[4] != 0;
  std::vector<double> cam, tgb, xyz_seq;
  std::vector<uint8_t> frames;
  std::vector<int32_t> i_seq;
  if (!read_n(f, &cam, 11) || !read_n(f, &tgb, 7 * F) || !read_n(f, &frames, F * W * H) ||
      !read_n(f, &xyz_seq, 3 * n_seq) || !read_n(f, &i_seq, n_seq))
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
  Cloud plain_cloud, batch_cloud;
  std::vector<int> plain_i, batch_i;
  std::vector<uint8_t> plain_pc2, batch_pc2;
  {
    stereo::Stereo plain(ncameras, settings, bmp);
    plain.addFrames(poses, images, &plain_cloud, &plain_i);
    plain_pc2 = plain.pointCloud2Payload();
  }
  {
    stereo::Stereo batched(ncameras, settings, bmp);
    batched.setPairsInFlight(3);
    batched.addFrames(poses, images, &batch_cloud, &batch_i);
    batch_pc2 = batched.pointCloud2Payload();
  }
  bad += compare("default object", plain_cloud, plain_i, xyz_seq, i_seq);
  bad += compare("setPairsInFlight(3)", batch_cloud, batch_i, xyz_seq, i_seq);
  if (plain_pc2.size() != W * H * 16 || plain_pc2 != batch_pc2) {
    std::printf("PointCloud2 payloads differ\n");
    ++bad;
  }
  std::printf(bad ? "FAILED\n" : "OK\n");
  return bad ? 1 : 0;
}
