// owned_check.cpp — csrc/device_owned.h, unchanged, over stand-ins for the HIP names it and this program use: malloc / free
// behind every handle, and counts of what was made and released.  A stand-alone program (tests/test_device_owned.py builds
// it with the address and undefined-behaviour sanitizers): a double release or a use after one ends it there, a leak shows
// in the counts and in the sanitizer's leak report.  Exit status 0 and a last line "... 0 live" when every check holds.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <string>
#include <type_traits>
#include <vector>

// ---- the stand-ins
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
constexpr hipError_t hipErrorInvalidValue = 1;
typedef struct StandInEvent* hipEvent_t;
typedef struct StandInStream* hipStream_t;

enum Kind { kDevice, kPinned, kEvent, kStream, kKinds };
static const char* const kKindName[kKinds] = {"device", "pinned", "event", "stream"};
static long g_made[kKinds], g_released[kKinds];
static std::vector<std::string> g_log;   // what was released, in order, when non-empty names were given

// every handle is a small heap block that names its kind: the sanitizer sees a double or a missing release
struct Block {
  Kind kind;
  const char* name;
};
static void* make(Kind k) {
  Block* b = (Block*)malloc(sizeof(Block));
  b->kind = k;
  b->name = nullptr;
  g_made[k]++;
  return b;
}
static hipError_t release(void* p, Kind k) {
  Block* b = (Block*)p;
  if (!b || b->kind != k) return hipErrorInvalidValue;
  if (b->name) g_log.push_back(b->name);
  g_released[k]++;
  free(b);
  return hipSuccess;
}
static void name_handle(void* p, const char* name) { ((Block*)p)->name = name; }

hipError_t hipMalloc(void** p, size_t) { return *p = make(kDevice), hipSuccess; }
hipError_t hipFree(void* p) { return release(p, kDevice); }
hipError_t hipHostMalloc(void** p, size_t, unsigned) { return *p = make(kPinned), hipSuccess; }
hipError_t hipHostFree(void* p) { return release(p, kPinned); }
hipError_t hipEventCreate(hipEvent_t* e) { return *e = (hipEvent_t)make(kEvent), hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { return release(e, kEvent); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return *s = (hipStream_t)make(kStream), hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { return release(s, kStream); }

#include "../../webgpu-raytracer_amd/csrc/device_owned.h"

using namespace owned;

static int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      g_failed++;                                                       \
    }                                                                   \
  } while (0)

static_assert(!std::is_copy_constructible<DeviceBuffer>::value && !std::is_copy_assignable<DeviceBuffer>::value, "DeviceBuffer copies");
static_assert(!std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value, "Event copies");
static_assert(!std::is_copy_constructible<Stream>::value && !std::is_copy_assignable<Stream>::value, "Stream copies");
static_assert(!std::is_copy_constructible<Pinned>::value && !std::is_copy_assignable<Pinned>::value, "Pinned copies");
static_assert(!std::is_copy_constructible<EventPair>::value && !std::is_copy_assignable<EventPair>::value, "EventPair copies");
static_assert(std::is_nothrow_move_constructible<DeviceBuffer>::value && std::is_nothrow_move_assignable<DeviceBuffer>::value, "DeviceBuffer moves");
static_assert(std::is_nothrow_move_constructible<EventPair>::value && std::is_nothrow_move_assignable<EventPair>::value, "EventPair moves");

// one owner type: how to fill an empty one, and whether one is empty
struct BufferOps {
  typedef DeviceBuffer Owner;
  static const Kind kind = kDevice;
  static void fill(DeviceBuffer& b) {
    CHECK(hipMalloc(&b.ptr, 64) == hipSuccess);
    b.capacity = 64;
    b.size = 48;
  }
  static bool empty(const DeviceBuffer& b) { return !b.ptr && b.capacity == 0 && b.size == 0; }
  static bool full(const DeviceBuffer& b) { return b.ptr && b.capacity == 64 && b.size == 48; }
  static void reset(DeviceBuffer& b) { b.reset(); }
};
struct EventOps {
  typedef Event Owner;
  static const Kind kind = kEvent;
  static void fill(Event& e) { CHECK(hipEventCreateWithFlags(&e, 2) == hipSuccess); }
  static bool empty(const Event& e) { return !e; }
  static bool full(const Event& e) { return e.h != nullptr && (hipEvent_t)e == e.h; }
  static void reset(Event& e) { CHECK(e.reset() == hipSuccess); }
};
struct StreamOps {
  typedef Stream Owner;
  static const Kind kind = kStream;
  static void fill(Stream& s) { CHECK(hipStreamCreateWithFlags(&s, 1) == hipSuccess); }
  static bool empty(const Stream& s) { return !s; }
  static bool full(const Stream& s) { return s.h != nullptr; }
  static void reset(Stream& s) { CHECK(s.reset() == hipSuccess); }
};
struct PinnedOps {
  typedef Pinned Owner;
  static const Kind kind = kPinned;
  static void fill(Pinned& p) { CHECK(hipHostMalloc(&p, 256, 0) == hipSuccess); }
  static bool empty(const Pinned& p) { return !p; }
  static bool full(const Pinned& p) { return p.h != nullptr; }
  static void reset(Pinned& p) { CHECK(p.reset() == hipSuccess); }
};

template <class Ops>
static void check_owner() {
  typedef typename Ops::Owner Owner;
  long& made = g_made[Ops::kind];
  long& released = g_released[Ops::kind];
  const long made0 = made, released0 = released;
  {  // a default-constructed owner frees nothing, and resetting it does not either
    Owner o;
    CHECK(Ops::empty(o));
    Ops::reset(o);
  }
  CHECK(made == made0 && released == released0);
  {  // destruction frees exactly once
    Owner o;
    Ops::fill(o);
    CHECK(Ops::full(o) && made == made0 + 1 && released == released0);
  }
  CHECK(released == released0 + 1);
  {  // reset() twice frees once
    Owner o;
    Ops::fill(o);
    Ops::reset(o);
    CHECK(Ops::empty(o) && released == released0 + 2);
    Ops::reset(o);
    CHECK(released == released0 + 2);
  }
  CHECK(released == released0 + 2);
  {  // move construction transfers ownership
    Owner a;
    Ops::fill(a);
    Owner b(std::move(a));
    CHECK(Ops::empty(a) && Ops::full(b) && released == released0 + 2);
  }
  CHECK(released == released0 + 3);
  {  // move assignment frees the overwritten target once and transfers ownership; onto itself it does nothing
    Owner a, b;
    Ops::fill(a);
    Ops::fill(b);
    b = std::move(a);
    CHECK(Ops::empty(a) && Ops::full(b) && released == released0 + 4);
    Owner& same = b;
    b = std::move(same);
    CHECK(Ops::full(b) && released == released0 + 4);
    a = std::move(b);   // into an empty target
    CHECK(Ops::full(a) && Ops::empty(b) && released == released0 + 4);
  }
  CHECK(released == released0 + 5 && made == made0 + 5);
}

static void check_pair_deque() {
  const long made0 = g_made[kEvent], released0 = g_released[kEvent];
  {
    std::deque<EventPair> pool;
    std::vector<const EventPair*> where;
    for (int k = 0; k < 300; k++) {   // several blocks of the deque
      EventPair& p = pool.emplace_back();
      CHECK(!p.a && !p.b);
      CHECK(hipEventCreate(&p.a) == hipSuccess && hipEventCreate(&p.b) == hipSuccess);
      where.push_back(&pool.back());
    }
    for (int k = 0; k < 300; k++) CHECK(where[k] == &pool[k] && pool[k].a && pool[k].b);   // a pair never moves
    pool.pop_back();   // next_events' way out of a failed create
    CHECK(g_released[kEvent] == released0 + 2);
    EventPair taken(std::move(pool[7]));   // a pair moves as its events do
    CHECK(!pool[7].a && !pool[7].b && taken.a && taken.b);
  }
  CHECK(g_made[kEvent] == made0 + 600 && g_released[kEvent] == released0 + 600);
}

// members go in reverse order of declaration: a context's streams, declared first, outlive its buffers and events
struct Context {
  Stream stream;
  DeviceBuffer buffer;
  Event event;
};
static void check_member_order() {
  {
    Context c;
    StreamOps::fill(c.stream);
    BufferOps::fill(c.buffer);
    EventOps::fill(c.event);
    name_handle(c.stream.h, "stream");
    name_handle(c.buffer.ptr, "buffer");
    name_handle(c.event.h, "event");
    g_log.clear();
  }
  CHECK((g_log == std::vector<std::string>{"event", "buffer", "stream"}));
  g_log.clear();
}

int main() {
  check_owner<BufferOps>();
  check_owner<EventOps>();
  check_owner<StreamOps>();
  check_owner<PinnedOps>();
  check_pair_deque();
  check_member_order();
  long live = 0;
  for (int k = 0; k < kKinds; k++) {
    printf("%s: %ld made, %ld released\n", kKindName[k], g_made[k], g_released[k]);
    CHECK(g_made[k] > 0);
    live += g_made[k] - g_released[k];
  }
  if (g_failed) {
    printf("owned_check: %d checks FAILED, %ld live\n", g_failed, live);
    return 1;
  }
  printf("owned_check: every check held, %ld live\n", live);
  return live == 0 ? 0 : 1;
}
