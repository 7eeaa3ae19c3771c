// reference: src/theia/sfm/create_and_initialize_ransac_variant.h:51-56 -- the enum only; of its values the device
// path provides RANSAC.
#ifndef THEIA_MI355_SFM_CREATE_AND_INITIALIZE_RANSAC_VARIANT_H_
#define THEIA_MI355_SFM_CREATE_AND_INITIALIZE_RANSAC_VARIANT_H_
namespace theia {
enum class RansacType {
  RANSAC = 0,
  PROSAC = 1,
  LMED = 2,
  EXHAUSTIVE = 3,
};
}  // namespace theia
#endif
