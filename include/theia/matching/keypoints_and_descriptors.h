// reference: src/theia/matching/keypoints_and_descriptors.h:48-52 -- the keypoints and descriptors of one image.
#ifndef THEIA_MI355_MATCHING_KEYPOINTS_AND_DESCRIPTORS_H_
#define THEIA_MI355_MATCHING_KEYPOINTS_AND_DESCRIPTORS_H_
#include <string>
#include <vector>

#include "theia/image/keypoint_detector/keypoint.h"
#include "theia/util/eigen_lite.h"
namespace theia {
struct KeypointsAndDescriptors {
  std::string image_name;
  std::vector<Keypoint> keypoints;
  std::vector<Eigen::VectorXf> descriptors;
};
}  // namespace theia
#endif
