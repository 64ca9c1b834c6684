// ictr_p2p.hip -- one-shot peer-to-peer all-reduce of the per-problem 27-float records.
//
// The sharded Gauss-Newton loop exchanges B x 27 floats per iteration (H 21 + b 6 per problem). For a message of a
// few KB a ring / tree collective is pure latency: 2 (N - 1) hops over point-to-point xGMI links. Every GPU of a
// node has a direct link to every other one, so the latency-optimal exchange is ONE hop: each rank stores its
// record straight into a mailbox slot in every peer's memory (mapped with hipIpc), then adds up the N slots of its
// own mailbox in rank order. No communicator, no proxy thread, no second stream: one small kernel enqueued on the
// compute stream between the tail and the finish kernels.
//
// The protocol is the one of ictr_xchg.h (granules, parity slots, bounded polling) over the rank mailbox layout, with
// system-scope stores and loads; the tag is the object's sequence number, the sticky error flag lives in device memory.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>

#include "ictr_dev.h"
#include "ictr_launch.h"

namespace ictr {

constexpr int kP2PMaxWorld = 16;

struct P2PArgs {
  uint64_t *peer[kP2PMaxWorld];  // every rank's mailbox as mapped into this process (own rank: the local pointer)
  uint64_t *local;
  int rank, world;
  int64_t cap;                // granules per slot
  int *err;                   // sticky device flag: an exchange timed out
  unsigned long long limit;   // polling limit in wall_clock64 ticks
};

__global__ __launch_bounds__(256) void k_p2p_allreduce(P2PArgs a, float *buf, int count, unsigned seq) {
  const size_t par = rank_mail_slot(seq, a.world);
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    const uint64_t g = xchg_pack(seq, buf[i]);
    for (int r = 0; r < a.world; ++r)  // my record into slot [rank] of every mailbox, mine included
      __hip_atomic_store(a.peer[r] + rank_mail_index(par + a.rank, a.cap, i), g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // this kernel's own variant of the time-out step (xchg_timed_out): the clock starts before the first load, the flag
  // is a device word raised by every lane that gives up, and there is no dead state -- one exchange per launch
  const unsigned long long t0 = wall_clock64();
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    float sum = 0.0f;
    for (int r = 0; r < a.world; ++r) {
      const uint64_t *src = a.local + rank_mail_index(par + r, a.cap, i);
      uint64_t g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      while (xchg_miss(g, seq)) {
        if (wall_clock64() - t0 > a.limit) {  // a peer never arrived: give up, flag it, leave the kernel
          atomicExch(a.err, 1);
          g = xchg_empty(seq);
          break;
        }
        __builtin_amdgcn_s_sleep(2);
        g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      sum += xchg_value(g);  // rank order: the same bits on every rank
    }
    buf[i] = sum;
  }
}

}  // namespace ictr

using namespace ictr;

struct ictr_p2p {
  int rank = 0, world = 1;
  int64_t cap = 0;
  DevBuf<uint64_t> mail;
  uint64_t *peer[kP2PMaxWorld] = {};  // peer[rank] = mail; the others are opened IPC handles
  bool opened[kP2PMaxWorld] = {};
  DevBuf<int> d_err;
  unsigned seq = 0;
  bool connected = false;
  double timeout_s = 2.0;
  ~ictr_p2p() {  // the peers' mailboxes are closed before this rank's own goes
    (void)hipDeviceSynchronize();
    for (int r = 0; r < world; ++r)
      if (opened[r] && peer[r]) (void)hipIpcCloseMemHandle(peer[r]);
  }
};

extern "C" int ictr_p2p_create(ictr_p2p **out, int rank, int world, int64_t count) {
  if (!out || world < 1 || world > kP2PMaxWorld || rank < 0 || rank >= world || count < 1 || count > (1 << 24))
    return fail(ICTR_ERR_INVALID, "p2p_create: bad arguments (world 1..%d)", kP2PMaxWorld);
  if (int rc = need_device()) return rc;
  auto p = std::make_unique<ictr_p2p>();
  p->rank = rank;
  p->world = world;
  p->cap = (count + 31) / 32 * 32;
  const size_t bytes = sizeof(uint64_t) * rank_mail_granules(world, p->cap);
  // mailbox memory that remote stores and local polls see coherently: uncached (fine-grained) device memory
  uint64_t *mail = nullptr;
  hipError_t e = hipExtMallocWithFlags((void **)&mail, bytes, hipDeviceMallocUncached);
  if (e != hipSuccess) e = hipExtMallocWithFlags((void **)&mail, bytes, hipDeviceMallocFinegrained);
  if (e != hipSuccess) return fail(ICTR_ERR_HIP, "p2p_create: mailbox allocation failed: %s", hipGetErrorString(e));
  p->mail.adopt(mail);
  HIPCHK(hipMemset(mail, 0, bytes));  // tag 0 = "nothing yet"; sequence numbers start at 1
  if (int rc = p->d_err.alloc(sizeof(int), true)) return rc;
  HIPCHK(hipDeviceSynchronize());
  if (const char *t = getenv("ICTR_P2P_TIMEOUT_S")) p->timeout_s = std::max(0.01, atof(t));
  p->peer[rank] = mail;
  *out = p.release();
  return ICTR_OK;
}

extern "C" int ictr_p2p_handle_bytes(void) { return (int)sizeof(hipIpcMemHandle_t); }

// the handle other processes open to reach this rank's mailbox (hipIpcMemHandle_t, ictr_p2p_handle_bytes() bytes)
extern "C" int ictr_p2p_local_handle(ictr_p2p *p, void *handle_out) {
  if (!p || !handle_out) return fail(ICTR_ERR_INVALID, "p2p_local_handle: NULL argument");
  hipIpcMemHandle_t h;
  HIPCHK(hipIpcGetMemHandle(&h, p->mail.get()));
  memcpy(handle_out, &h, sizeof(h));
  return ICTR_OK;
}

// all_handles: world handles in rank order (this rank's own entry is ignored)
extern "C" int ictr_p2p_connect(ictr_p2p *p, const void *all_handles) {
  if (!p || !all_handles) return fail(ICTR_ERR_INVALID, "p2p_connect: NULL argument");
  for (int r = 0; r < p->world; ++r) {
    if (r == p->rank || p->opened[r]) continue;
    hipIpcMemHandle_t h;
    memcpy(&h, (const char *)all_handles + (size_t)r * sizeof(h), sizeof(h));
    void *ptr = nullptr;
    HIPCHK(hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess));
    p->peer[r] = (uint64_t *)ptr;
    p->opened[r] = true;
  }
  p->connected = true;
  return ICTR_OK;
}

// in-place sum of dev_buf[0..count) over all ranks, enqueued on `hip_stream`; every rank must call it the same
// number of times with the same count
extern "C" int ictr_p2p_allreduce(ictr_p2p *p, float *dev_buf, int64_t count, void *hip_stream) {
  if (!p || !dev_buf || count < 1 || count > p->cap) return fail(ICTR_ERR_INVALID, "p2p_allreduce: bad arguments");
  if (!p->connected && p->world > 1) return fail(ICTR_ERR_STATE, "p2p_allreduce before p2p_connect");
  P2PArgs a;
  memset(&a, 0, sizeof(a));
  for (int r = 0; r < p->world; ++r) a.peer[r] = p->peer[r];
  a.local = p->mail.get();
  a.rank = p->rank;
  a.world = p->world;
  a.cap = p->cap;
  a.err = p->d_err.get();
  a.limit = (unsigned long long)(p->timeout_s * kWallClockHz);
  p->seq += 1;
  if (p->seq == 0) p->seq = 1;  // tag 0 is reserved for "empty"
  hipLaunchKernelGGL(k_p2p_allreduce, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, a, dev_buf, (int)count, p->seq);
  HIPCHK(hipGetLastError());
  return ICTR_OK;
}

// internal (ictr_host.hip): the mailboxes as a kernel argument of the resident-iteration launch (sharded resident form)
extern "C" int ictr_p2p_fill_xchg_(const ictr_p2p *p, ictr::ResXchg *x) {
  if (!p || !x || (!p->connected && p->world > 1)) return 1;
  memset(x, 0, sizeof(*x));
  for (int r = 0; r < p->world; ++r) x->peer[r] = (unsigned long long *)p->peer[r];
  x->local = (unsigned long long *)p->mail.get();
  x->rank = p->rank;
  x->world = p->world;
  x->cap = p->cap;
  return 0;
}

// 0: every exchange so far completed; 1: one timed out (a peer did not arrive). Synchronises the device.
extern "C" int ictr_p2p_error(ictr_p2p *p) {
  if (!p) return 1;
  int e = 1;
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpy(&e, p->d_err.get(), sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  return e;
}

extern "C" void ictr_p2p_destroy(ictr_p2p *p) { delete p; }
