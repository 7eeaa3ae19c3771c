// reference: src/theia/image/keypoint_detector/keypoint.h:50-116 -- a detected keypoint: position, type and the
// optional strength, scale and orientation (unset = THEIA_INVALID_KEYPOINT_VAR).  Serialisation is not provided.
#ifndef THEIA_MI355_IMAGE_KEYPOINT_DETECTOR_KEYPOINT_H_
#define THEIA_MI355_IMAGE_KEYPOINT_DETECTOR_KEYPOINT_H_
namespace theia {
#define THEIA_INVALID_KEYPOINT_VAR -9999
class Keypoint {
 public:
  enum KeypointType { INVALID = -1, OTHER = 0, SIFT = 1, AKAZE = 2 };
  Keypoint(double x, double y, KeypointType type) : x_(x), y_(y), keypoint_type_(type) {}
  Keypoint() : Keypoint(THEIA_INVALID_KEYPOINT_VAR, THEIA_INVALID_KEYPOINT_VAR, Keypoint::INVALID) {}
  KeypointType keypoint_type() const { return keypoint_type_; }
  void set_keypoint_type(KeypointType type) { keypoint_type_ = type; }
  double x() const { return x_; }
  void set_x(double x) { x_ = x; }
  double y() const { return y_; }
  void set_y(double y) { y_ = y; }
  bool has_strength() const { return strength_ != THEIA_INVALID_KEYPOINT_VAR; }
  double strength() const { return strength_; }
  void set_strength(double strength) { strength_ = strength; }
  bool has_scale() const { return scale_ != THEIA_INVALID_KEYPOINT_VAR; }
  double scale() const { return scale_; }
  void set_scale(double scale) { scale_ = scale; }
  bool has_orientation() const { return orientation_ != THEIA_INVALID_KEYPOINT_VAR; }
  double orientation() const { return orientation_; }
  void set_orientation(double orientation) { orientation_ = orientation; }

 private:
  double x_, y_;
  KeypointType keypoint_type_;
  double strength_ = THEIA_INVALID_KEYPOINT_VAR;
  double scale_ = THEIA_INVALID_KEYPOINT_VAR;
  double orientation_ = THEIA_INVALID_KEYPOINT_VAR;
};
}  // namespace theia
#endif
