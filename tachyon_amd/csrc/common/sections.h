// The host image of a "one upload" buffer: sections laid one after another,
// each starting on a 16-byte boundary (host code only, no HIP).
#pragma once
#include <cstddef>
#include <vector>

namespace tachyon_amd {

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

class SectionPacker {
 public:
  void reset() { size_ = 0; }
  // The offset of a new section of `bytes` bytes (which may be none)
  size_t add(size_t bytes) {
    const size_t at = align16(size_);
    size_ = at + bytes;
    return at;
  }
  size_t size() const { return size_; }
  // The image, zeroed, once every section is added; it stays where it is
  // until the next call
  unsigned char* image() {
    bytes_.assign(size_ ? size_ : 1, 0);
    return bytes_.data();
  }
  const unsigned char* data() const { return bytes_.data(); }

 private:
  size_t size_ = 0;
  std::vector<unsigned char> bytes_;
};

}  // namespace tachyon_amd
