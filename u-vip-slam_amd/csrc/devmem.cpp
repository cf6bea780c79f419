// hipMalloc / hipHostMalloc and their frees for every handle of the library except the matcher's slot set (devmem.hpp, common.hpp).
#include "devmem.hpp"

namespace uvo {

int dev_malloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) return UVO_OK;
  *p = nullptr;
  hip_err_set(e, "hipMalloc");
  return e == hipErrorOutOfMemory ? UVO_E_NOMEM : UVO_E_HIP;
}

int DevMem::alloc_bytes(void** p, size_t bytes, bool pinned) {
  *p = nullptr;
  if (!pinned) RC(dev_malloc(p, bytes));
  else if (hipHostMalloc(p, bytes, hipHostMallocDefault) != hipSuccess) return *p = nullptr, fail(UVO_E_NOMEM, "pinned staging allocation failed");
  blocks.push_back(Block{*p, bytes, pinned});
  return UVO_OK;
}
size_t DevMem::bytes_of(const void* p) const {
  for (const Block& b : blocks)
    if (b.p == p) return b.bytes;
  return 0;
}
void DevMem::release(void* p) {
  for (size_t i = 0; i < blocks.size(); ++i)
    if (blocks[i].p == p) {
      (void)(blocks[i].pinned ? hipHostFree(p) : hipFree(p));
      blocks.erase(blocks.begin() + i);
      return;
    }
}
void DevMem::release_all() {
  while (!blocks.empty()) release(blocks.back().p);
}

}  // namespace uvo
