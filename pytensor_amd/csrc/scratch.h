// scratch.h — scope guard for library scratch taken from the pool (pthip_alloc / pthip_free).
// Depends on include/pthip.h only, so a plain host compiler can build it.
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/pthip.h"

namespace pthip {

// Owns any number of pool blocks and returns every one of them when it goes out of scope, so each
// way out of a function frees.  Freeing while the kernels that use a block are still queued is
// safe: reuse is stream-ordered (one in-order stream), so whatever is handed the block next runs
// after them.  pthip_free cannot fail here: it rejects only unknown or already-freed pointers,
// and each block held is live and freed exactly once.
class Scratch {
 public:
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() { release(); }

  // returns every block now, for a function that goes on to a callee with scratch of its own
  void release() {
    for (void* b : blocks_) pthip_free(b);
    blocks_.clear();
  }

  int alloc(size_t bytes, void** p) {
    *p = nullptr;
    const int r = pthip_alloc(bytes, p);
    if (*p) blocks_.push_back(*p);  // a block can be handed out although r != 0 (PTHIP_POISON's fill failed)
    return r;
  }

 private:
  std::vector<void*> blocks_;
};

}  // namespace pthip
