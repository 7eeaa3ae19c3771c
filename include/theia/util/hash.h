// reference: src/theia/util/hash.h -- std::hash for pairs, so that a ViewIdPair can key an unordered_map as it does
// throughout the reference (view_graph.h, rotation_estimator.h).  Only the pair of 32-bit ids is provided here.
#ifndef THEIA_MI355_UTIL_HASH_H_
#define THEIA_MI355_UTIL_HASH_H_
#include <cstddef>
#include <cstdint>
#include <functional>
#include <utility>

namespace std {
template <>
struct hash<std::pair<std::uint32_t, std::uint32_t>> {
  std::size_t operator()(const std::pair<std::uint32_t, std::uint32_t>& p) const {
    return std::hash<std::uint64_t>()((static_cast<std::uint64_t>(p.first) << 32) | p.second);
  }
};
}  // namespace std
#endif
