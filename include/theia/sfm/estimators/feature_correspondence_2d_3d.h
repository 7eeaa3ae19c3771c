// reference: src/theia/sfm/estimators/feature_correspondence_2d_3d.h:42-45 -- a (normalised) image feature and the
// world point it observes.
#ifndef THEIA_MI355_SFM_ESTIMATORS_FEATURE_CORRESPONDENCE_2D_3D_H_
#define THEIA_MI355_SFM_ESTIMATORS_FEATURE_CORRESPONDENCE_2D_3D_H_
#include "theia/util/eigen_lite.h"
namespace theia {
struct FeatureCorrespondence2D3D {
  Eigen::Vector2d feature;
  Eigen::Vector3d world_point;
};
}  // namespace theia
#endif
