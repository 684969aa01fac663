// Launch record of the C ABI (include/cdseg.h: cdseg_route_enable / _clear / _read / _catalog / _note); csrc/route.h.
// Host code only: no kernel, no device call.
#include <cstring>

#include "common.h"
#include "route.h"

thread_local bool tl_cdseg_route_on = false;

namespace {
constexpr int RING = 64;  // records kept per thread (a cdseg_block_forward leaves at most ten)
struct Ring {
  int32_t rec[RING][CDSEG_ROUTE_WORDS];
  long count = 0;  // launches recorded since the last clear
};
thread_local Ring tl_ring;
}  // namespace

void cdseg_route_push(int id, int bm, int bn, int splits, int fix, int xmode, int flags, int aux) {
  int32_t* r = tl_ring.rec[tl_ring.count % RING];
  r[CDSEG_ROUTE_ID] = id; r[CDSEG_ROUTE_BM] = bm; r[CDSEG_ROUTE_BN] = bn; r[CDSEG_ROUTE_SPLITS] = splits;
  r[CDSEG_ROUTE_FIX] = fix; r[CDSEG_ROUTE_XMODE] = xmode; r[CDSEG_ROUTE_FLAGS] = flags; r[CDSEG_ROUTE_AUX] = aux;
  ++tl_ring.count;
}

void cdseg_route_or_flags(int flags) {
  if (tl_cdseg_route_on && tl_ring.count > 0) tl_ring.rec[(tl_ring.count - 1) % RING][CDSEG_ROUTE_FLAGS] |= flags;
}

extern "C" int cdseg_route_enable(int on) {
  const int prev = tl_cdseg_route_on ? 1 : 0;
  tl_cdseg_route_on = on != 0;
  return prev;
}

extern "C" void cdseg_route_clear(void) { tl_ring.count = 0; }

extern "C" int cdseg_route_read(int32_t* rec, int capacity) {
  const long count = tl_ring.count;
  long take = count < RING ? count : RING;
  if (!rec || capacity <= 0) take = 0;
  if (take > capacity) take = capacity;
  for (long i = 0; i < take; ++i)
    memcpy(rec + i * CDSEG_ROUTE_WORDS, tl_ring.rec[(count - take + i) % RING], sizeof(tl_ring.rec[0]));
  return count > 0x7fffffffL ? 0x7fffffff : (int)count;
}

extern "C" int cdseg_route_catalog(char* buf, size_t bytes) {
  size_t need = 0;
  for (int i = 0; i < kCdsegRouteCount; ++i) need += strlen(kCdsegRouteTable[i].name) + 1;  // '\n', the last one '\0'
  if (buf && bytes >= need) {
    char* q = buf;
    for (int i = 0; i < kCdsegRouteCount; ++i) {
      const size_t n = strlen(kCdsegRouteTable[i].name);
      memcpy(q, kCdsegRouteTable[i].name, n);
      q += n;
      *q++ = i + 1 < kCdsegRouteCount ? '\n' : '\0';
    }
  }
  return (int)need;
}

extern "C" int cdseg_route_note(const int32_t* rec) {
  if (!rec) return CDSEG_ERR_ARG;
  if (rec[CDSEG_ROUTE_ID] < 0 || rec[CDSEG_ROUTE_ID] >= kCdsegRouteCount) return CDSEG_ERR_ARG;
  cdseg_route_rec(rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7]);
  return CDSEG_OK;
}
