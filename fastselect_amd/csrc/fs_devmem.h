// fs_devmem.h -- the two owners of device memory, on top of the device block
// cache (dev_alloc / dev_free, fs_gpu_mem.hip).  A DevArena owns blocks that
// share one lifetime and frees them together; a DevBuf owns one block that
// grows on demand.  Whoever releases an arena has synchronised the streams
// that use its blocks; DevBuf::reserve does that itself before it frees.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "fs_internal.h"

namespace fs {
namespace gpu {

struct DevArena {
  int device;
  std::vector<void*> blocks;
  explicit DevArena(int dev) : device(dev) {}
  DevArena(const DevArena&) = delete;
  DevArena& operator=(const DevArena&) = delete;
  ~DevArena() { release(); }
  template <class T>
  int alloc(T** p, size_t count) {
    void* q = nullptr;
    if (count == 0) count = 1;
    if (int rc = dev_alloc(&q, count * sizeof(T), device)) return rc;
    blocks.push_back(q);
    *p = (T*)q;
    return FS_OK;
  }
  void release() {  // the caller synchronised the streams that use the blocks
    for (void* q : blocks) dev_free(q);
    blocks.clear();
  }
};

template <class T>
struct DevBuf {
  int device;
  T* p = nullptr;
  size_t cap = 0;  // elements
  explicit DevBuf(int dev) : device(dev) {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  // At least `count` elements (count + slack when it has to grow; the
  // contents are not kept).  sync[0..nsync): every stream that may still use
  // the present block.
  int reserve(size_t count, size_t slack, hipStream_t* sync, int nsync) {
    if (count <= cap) return FS_OK;
    for (int k = 0; p && k < nsync; k++)
      if (hipError_t e = hipStreamSynchronize(sync[k]); e != hipSuccess) {
        set_error(std::string("HIP error '") + hipGetErrorString(e) + "' before a buffer grows");
        return FS_EHIP;
      }
    release();
    void* q = nullptr;
    if (int rc = dev_alloc(&q, (count + slack) * sizeof(T), device)) return rc;
    p = (T*)q;
    cap = count + slack;
    return FS_OK;
  }
  void release() {  // the caller synchronised the streams that use the block
    dev_free(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace gpu
}  // namespace fs
