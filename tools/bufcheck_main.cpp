// Stand-alone check of the owning buffer (mantis_amd/csrc/hostbuf.h) that holds
// a context's GPU and pinned memory, with a counting malloc policy that can be
// told to fail its k-th allocation: the rule of grow, the order of free and
// allocate, what a failure leaves, one free per block. A program of its own so
// that it can be built with sanitizers and run directly:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o build/bufcheck tools/bufcheck_main.cpp && build/bufcheck
// Exit status 0 and "bufcheck ok" when every case holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "../mantis_amd/csrc/hostbuf.h"

static int g_fail = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      g_fail++;                                                      \
    }                                                                \
  } while (0)

// malloc / free that count, log their order and fail allocation number fail_at (1-based; 0: never)
struct Counting {
  static int allocs, frees, live, fail_at;
  static size_t last_bytes;
  static std::string log;  // 'a' per allocation (also a failed one), 'f' per free
  static constexpr const char* kFailed = "counting malloc failed";
  static void* alloc(size_t bytes) {
    log += 'a';
    last_bytes = bytes;
    if (++allocs == fail_at) return nullptr;
    live++;
    return std::malloc(bytes);
  }
  static void free(void* p) {
    log += 'f';
    frees++;
    live--;
    std::free(p);
  }
  static void reset(int fail = 0) {
    allocs = frees = 0;
    fail_at = fail;
    last_bytes = 0;
    log.clear();
  }
};
int Counting::allocs, Counting::frees, Counting::live, Counting::fail_at;
size_t Counting::last_bytes;
std::string Counting::log;

struct Ctx {
  std::string err;
};
using Buf = mk::Buf<double, Counting>;

static_assert(!std::is_copy_constructible<Buf>::value, "a buffer must not be copy-constructed");
static_assert(!std::is_copy_assignable<Buf>::value, "a buffer must not be copy-assigned");
static_assert(!std::is_move_constructible<Buf>::value && !std::is_move_assignable<Buf>::value,
              "a buffer is not moved either: it is a member for the life of its context");

int main() {
  Ctx c;
  {  // from empty; equal and smaller counts; a larger count
    Counting::reset();
    Buf b;
    CHECK(b.get() == nullptr && b.capacity() == 0);
    CHECK(b.grow(&c, 0) == MANTIS_OK && b.get() == nullptr && Counting::allocs == 0);  // 0 <= capacity
    CHECK(b.grow(&c, 5) == MANTIS_OK && b.get() != nullptr && b.capacity() == 5);
    CHECK(Counting::log == "a" && Counting::last_bytes == 5 * sizeof(double));
    double* p = b;  // the conversion launches and copies use
    for (int i = 0; i < 5; i++) p[i] = i;  // the whole block is ours (AddressSanitizer)
    CHECK(b.grow(&c, 5) == MANTIS_OK && b.grow(&c, 3) == MANTIS_OK && b.grow(&c, 0) == MANTIS_OK);
    CHECK(b.get() == p && b.capacity() == 5 && Counting::log == "a");
    CHECK(b.grow(&c, 9) == MANTIS_OK && b.capacity() == 9);
    CHECK(Counting::log == "afa");  // the old block freed once, before the new allocation
    CHECK(Counting::last_bytes == 9 * sizeof(double) && Counting::live == 1);
    for (int i = 0; i < 9; i++) b[i] = i;
  }
  CHECK(Counting::log == "afaf" && Counting::live == 0);  // the destructor frees once

  {  // count 0 allocates one element; alloc() reallocates whatever the capacity
    Counting::reset();
    Buf b;
    CHECK(b.alloc(&c, 0) == MANTIS_OK && b.get() != nullptr && b.capacity() == 0);
    CHECK(Counting::last_bytes == sizeof(double));
    b[0] = 1.0;
    CHECK(b.alloc(&c, 0) == MANTIS_OK && Counting::log == "afa" && Counting::live == 1);
    b.release();
    b.release();  // idempotent
    CHECK(b.get() == nullptr && Counting::log == "afaf" && Counting::live == 0);
  }
  CHECK(Counting::log == "afaf");  // nothing left for the destructor

  {  // a failing allocation: empty, capacity 0, the error and the status; the next grow succeeds
    Counting::reset(2);
    Buf b;
    c.err.clear();
    CHECK(b.grow(&c, 4) == MANTIS_OK && c.err.empty());
    CHECK(b.grow(&c, 8) == MANTIS_ERR_OOM);
    CHECK(b.get() == nullptr && b.capacity() == 0 && c.err == Counting::kFailed);
    CHECK(Counting::log == "afa" && Counting::live == 0);  // the old block went before the attempt
    CHECK(b.grow(&c, 2) == MANTIS_OK && b.get() != nullptr && b.capacity() == 2 && Counting::live == 1);
  }
  CHECK(Counting::live == 0);

  {  // a failure in the middle of a chain of three, as the workspaces write it
    Counting::reset(2);
    Buf x, y, z;
    CHECK((x.grow(&c, 3) || y.grow(&c, 3) || z.grow(&c, 3)) == true);
    CHECK(x.get() != nullptr && x.capacity() == 3);
    CHECK(y.get() == nullptr && y.capacity() == 0);
    CHECK(z.get() == nullptr && z.capacity() == 0 && Counting::allocs == 2);  // never reached
    CHECK(Counting::live == 1);
    // the call after: only what is missing is allocated
    CHECK((x.grow(&c, 3) || y.grow(&c, 3) || z.grow(&c, 3)) == false);
    CHECK(Counting::allocs == 4 && Counting::frees == 0 && Counting::live == 3);
  }
  CHECK(Counting::frees == 3 && Counting::live == 0);  // all released at scope exit

  {  // as a call's scratch: a vector-free scope of buffers, an early exit in between
    Counting::reset();
    auto call = [&](bool fail_early) -> mantis_status {
      Buf a, b;
      if (a.alloc(&c, 7) || b.alloc(&c, 1)) return MANTIS_ERR_OOM;
      if (fail_early) return MANTIS_ERR_DEVICE;
      return MANTIS_OK;
    };
    CHECK(call(true) == MANTIS_ERR_DEVICE && Counting::live == 0);
    CHECK(call(false) == MANTIS_OK && Counting::live == 0 && Counting::allocs == 4 && Counting::frees == 4);
  }

  CHECK(Counting::live == 0);
  if (g_fail) {
    std::printf("bufcheck: %d failed\n", g_fail);
    return 1;
  }
  std::printf("bufcheck ok\n");
  return 0;
}
