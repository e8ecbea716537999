// TEST INFRASTRUCTURE ONLY.  pt::DevBuf (csrc/device/dev_buf.h) over the counting, malloc-backed hipMalloc / hipFree / hipMemcpy of this
// directory's <hip/hip_runtime.h>: a stand-alone program (tests/test_dev_buf_on_host.py builds it with -fsanitize=address,undefined and runs
// it), so a double free or a leak ends it as surely as a mismatch below does.  Exit status: the number of failed expectations.
#include "dev_buf.h"

#include <cstdio>
#include <type_traits>

using pt::DevBuf;

static int g_failed = 0;
#define EXPECT(cond)                                                                                                     \
  if(!(cond))                                                                                                            \
  {                                                                                                                     \
    std::fprintf(stderr, "%s:%d: expected %s\n", __FILE__, __LINE__, #cond);                                            \
    ++g_failed;                                                                                                         \
  }

static_assert(!std::is_copy_constructible_v<DevBuf<int>>, "a copy would free twice");
static_assert(!std::is_copy_assignable_v<DevBuf<int>>, "a copy would free twice");
static_assert(std::is_nothrow_move_constructible_v<DevBuf<int>> && std::is_nothrow_move_assignable_v<DevBuf<int>>, "move-only");

static long live() { return g_hipShim.mallocs - g_hipShim.frees; }

int main()
{
  {  // a move leaves the source empty, and the block is freed once
    DevBuf<int> a;
    EXPECT(a.alloc(10) == hipSuccess && a.ptr && a.count == 10 && a.bytes() == 40);
    int* const  block = a.ptr;
    DevBuf<int> b(std::move(a));
    EXPECT(a.ptr == nullptr && a.count == 0 && a.bytes() == 0);
    EXPECT(b.ptr == block && b.count == 10);
    EXPECT(live() == 1);
  }
  EXPECT(live() == 0 && g_hipShim.mallocs == 1);
  {  // move assignment frees the target's old block once and empties the source; onto itself it changes nothing
    DevBuf<float> a, b;
    EXPECT(a.alloc(3) == hipSuccess && b.alloc(5) == hipSuccess);
    float* const block  = b.ptr;
    const long   before = g_hipShim.frees;
    a = std::move(b);
    EXPECT(g_hipShim.frees == before + 1);
    EXPECT(a.ptr == block && a.count == 5 && b.ptr == nullptr && b.count == 0);
    DevBuf<float>& same = a;
    a = std::move(same);
    EXPECT(a.ptr == block && a.count == 5 && g_hipShim.frees == before + 1);
    std::swap(a, b);  // (the builders' ping-pong pairs)
    EXPECT(b.ptr == block && b.count == 5 && a.ptr == nullptr && a.count == 0 && g_hipShim.frees == before + 1);
  }
  EXPECT(live() == 0);
  {  // release is idempotent; alloc over a held block releases it first; alloc(0) gives null and count 0
    DevBuf<int> a;
    a.release();
    EXPECT(a.alloc(4) == hipSuccess);
    const long before = g_hipShim.frees;
    EXPECT(a.alloc(8) == hipSuccess && g_hipShim.frees == before + 1 && a.count == 8);
    a.release();
    a.release();
    EXPECT(g_hipShim.frees == before + 2 && a.ptr == nullptr && a.count == 0);
    EXPECT(a.alloc(4) == hipSuccess);
    EXPECT(a.alloc(0) == hipSuccess && a.ptr == nullptr && a.count == 0 && a.bytes() == 0);
  }
  EXPECT(live() == 0);
  {  // a failed alloc gives null, count 0 and bytes() 0 -- also over a held block, which is gone by then
    DevBuf<double> a;
    g_hipShim.failAt = 1;
    EXPECT(a.alloc(7) == hipErrorOutOfMemory && a.ptr == nullptr && a.count == 0 && a.bytes() == 0);
    EXPECT(a.alloc(7) == hipSuccess && a.bytes() == 56);
    g_hipShim.failAt = 1;
    EXPECT(a.alloc(9) == hipErrorOutOfMemory && a.ptr == nullptr && a.count == 0 && a.bytes() == 0);
    // the n-th: the second of two
    DevBuf<double> b;
    g_hipShim.failAt = 2;
    EXPECT(a.alloc(2) == hipSuccess && b.alloc(2) == hipErrorOutOfMemory && a.count == 2 && b.count == 0);
  }
  EXPECT(live() == 0);
  {  // upload copies what it was given; a failed upload does not copy; an upload of nothing neither allocates nor copies
    const int   src[3] = {7, 8, 9};
    DevBuf<int> a;
    long        copies = g_hipShim.memcpys;
    EXPECT(a.upload(src, 3) == hipSuccess && g_hipShim.memcpys == copies + 1 && a.count == 3 && a.ptr[0] == 7 && a.ptr[2] == 9);
    copies           = g_hipShim.memcpys;
    g_hipShim.failAt = 1;
    EXPECT(a.upload(src, 3) == hipErrorOutOfMemory && g_hipShim.memcpys == copies && a.ptr == nullptr && a.count == 0);
    EXPECT(a.upload(src, 0) == hipSuccess && g_hipShim.memcpys == copies && a.ptr == nullptr && a.count == 0);
  }
  EXPECT(live() == 0 && g_hipShim.mallocs > 0);
  std::printf("dev_buf_on_host: %ld allocations, %ld frees, %d failed expectations\n", g_hipShim.mallocs, g_hipShim.frees, g_failed);
  return g_failed;
}
