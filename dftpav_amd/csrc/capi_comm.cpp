// capi_comm.cpp — RCCL behind the C-ABI.
#include <dlfcn.h>
#include <atomic>
#include <mutex>

#include "capi_internal.h"

// An RCCL communicator and the number of handles that hold it (its creator and the handles it was shared with, each on its own
// host thread at most): the communicator is destroyed by whichever of them lets go last, in whatever order they do.  An RCCL
// communicator does not take concurrent enqueues: `mu` is held around every call on it (the holders' threads serialise there;
// the ORDER of the collectives across ranks stays the host's business -- same order on every rank).  Taking and dropping a
// reference (share / destroy / create) happens under g_comm_mu, so a handle never reads another's comm_ref while that one
// lets go of it.
struct CommShared {
  void *comm;
  std::atomic<int> holders;
  std::mutex mu;
};
static std::mutex g_comm_mu;

// ------------------------------------------------------------------ RCCL behind the C-ABI
// The one collective of the path: an all-gather of 16-byte result records over xGMI.  RCCL is loaded at the first use
// (dlopen by its soname: inside a process that already holds an RCCL -- PyTorch ships one -- this is that same copy, so a
// process never runs two), which keeps the library loadable where no RCCL is installed: only these entry points fail there.
namespace {
struct RcclUniqueId {
  char internal[DFTPAV_UNIQUE_ID_BYTES];
};
struct RcclApi {
  void *lib = nullptr;
  int (*GetUniqueId)(RcclUniqueId *) = nullptr;
  int (*CommInitRank)(void **, int, RcclUniqueId, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  bool ok = false;
};
RcclApi &rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (api.lib) break;
    }
    if (!api.lib) return;
    api.GetUniqueId = reinterpret_cast<int (*)(RcclUniqueId *)>(dlsym(api.lib, "ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<int (*)(void **, int, RcclUniqueId, int)>(dlsym(api.lib, "ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<int (*)(void *)>(dlsym(api.lib, "ncclCommDestroy"));
    api.AllGather = reinterpret_cast<int (*)(const void *, void *, size_t, int, void *, hipStream_t)>(dlsym(api.lib, "ncclAllGather"));
    api.GetErrorString = reinterpret_cast<const char *(*)(int)>(dlsym(api.lib, "ncclGetErrorString"));
    api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllGather;
  });
  return api;
}
constexpr int kNcclUint8 = 1; // ncclUint8 == ncclChar + 1 (rccl.h)
} // namespace
#define RCCLCHK(h, call)                                                                                        \
  do {                                                                                                          \
    int e_ = (call);                                                                                            \
    if (e_ != 0) {                                                                                              \
      (h)->err = std::string(#call) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(e_) : "rccl error"); \
      return DFTPAV_E_COMM;                                                                                     \
    }                                                                                                           \
  } while (0)

extern "C" int dftpav_comm_unique_id(void *id) {
  if (!id) return DFTPAV_E_INVALID;
  if (!rccl().ok) return DFTPAV_E_COMM;
  RcclUniqueId u;
  if (rccl().GetUniqueId(&u) != 0) return DFTPAV_E_COMM;
  std::memcpy(id, u.internal, DFTPAV_UNIQUE_ID_BYTES);
  return DFTPAV_OK;
}
// Is RCCL loadable here?  (dlopen + dlsym only: no bootstrap root is started, unlike dftpav_comm_unique_id.)
extern "C" int dftpav_comm_available(void) { return rccl().ok ? 1 : 0; }
// lets go of h's reference to its communicator; g_comm_mu is held by the caller, h's stream is drained
static void comm_release_locked(dftpav_handle *h) {
  if (h->comm_ref && h->comm_ref->holders.fetch_sub(1) == 1) { // the last holder (every holder has drained its own stream)
    {
      std::lock_guard<std::mutex> lk(h->comm_ref->mu);
      (void)rccl().CommDestroy(h->comm_ref->comm);
    }
    delete h->comm_ref;
  }
  h->comm = nullptr;
  h->comm_ref = nullptr;
}
extern "C" int dftpav_comm_destroy(dftpav_handle *h) {
  if (!h) return DFTPAV_E_INVALID;
  if (h->comm) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    std::lock_guard<std::mutex> reg(g_comm_mu);
    comm_release_locked(h);
  }
  if (h->d_comm_send) (void)hipFree(h->d_comm_send);
  h->d_comm_send = nullptr;
  h->comm_send_bytes = 0;
  h->comm_ranks = 0;
  return DFTPAV_OK;
}
extern "C" int dftpav_comm_create(dftpav_handle *h, int nranks, int rank, const void *unique_id) {
  if (!h || nranks < 1 || rank < 0 || rank >= nranks || !unique_id) return DFTPAV_E_INVALID;
  if (!rccl().ok) {
    h->err = "RCCL (librccl.so.1) is not loadable";
    return DFTPAV_E_COMM;
  }
  if (int rc = dftpav_comm_destroy(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  RcclUniqueId u;
  std::memcpy(u.internal, unique_id, DFTPAV_UNIQUE_ID_BYTES);
  RCCLCHK(h, rccl().CommInitRank(&h->comm, nranks, u, rank));
  {
    std::lock_guard<std::mutex> reg(g_comm_mu);
    h->comm_ref = new CommShared;
    h->comm_ref->comm = h->comm;
    h->comm_ref->holders.store(1);
  }
  h->comm_ranks = nranks;
  h->comm_rank = rank;
  return DFTPAV_OK;
}
// Several handles (= HIP streams) of one process on one communicator: a host that keeps k batches in flight on k handles sets
// ONE communicator up per rank instead of k (k ncclCommInitRank rendezvous and k sets of RCCL buffers per rank otherwise).
// RCCL orders successive operations of a communicator among the streams they are enqueued on; what the host owes it is the
// same order of collectives on every rank -- which a round-robin over the handles is.
extern "C" int dftpav_comm_share(dftpav_handle *h, dftpav_handle *owner) {
  if (!h || !owner || h == owner) return DFTPAV_E_INVALID;
  // h's stream is drained BEFORE the registry lock is taken (its collectives may still be in flight on the communicator it gives up)
  if (h->comm) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
  }
  std::lock_guard<std::mutex> reg(g_comm_mu);
  if (owner->comm && owner->comm_ref && owner->comm_ref == h->comm_ref) return DFTPAV_OK; // already the same communicator
  // the owner is checked and the new reference taken FIRST: a share that fails leaves h as it was (round 5 released h's own
  // communicator before the check -- a failed share could then destroy it on this rank alone and hang the other ranks)
  if (!owner->comm || !owner->comm_ref || owner->device != h->device) { // read under the lock: the owner may be letting go
    h->err = "dftpav_comm_share: the other handle needs a communicator (dftpav_comm_create, or shared itself) on the same device";
    return DFTPAV_E_INVALID;
  }
  owner->comm_ref->holders.fetch_add(1);
  if (h->comm) comm_release_locked(h); // ... only then the old one goes
  if (h->d_comm_send) (void)hipFree(h->d_comm_send); // (sized for the communicator it belonged to)
  h->d_comm_send = nullptr;
  h->comm_send_bytes = 0;
  h->comm = owner->comm;
  h->comm_ref = owner->comm_ref;
  h->comm_ranks = owner->comm_ranks;
  h->comm_rank = owner->comm_rank;
  return DFTPAV_OK;
}
extern "C" int dftpav_comm_layout(int global_B, int nranks, int rank, int *first, int *count, int *block) {
  if (global_B < 1 || nranks < 1 || rank < 0 || rank >= nranks) return DFTPAV_E_INVALID;
  const long long lo = (long long)global_B * rank / nranks, hi = (long long)global_B * (rank + 1) / nranks;
  if (first) *first = (int)lo;
  if (count) *count = (int)(hi - lo);
  if (block) *block = (global_B + nranks - 1) / nranks; // the largest shard: every rank's block in the gathered buffer
  return DFTPAV_OK;
}
extern "C" int dftpav_batch_allgather_results(dftpav_batch *b, int global_B, void *all_records) {
  if (!b || !all_records || !b->uploaded || !b->solved) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  if (!h->comm) {
    h->err = "dftpav_comm_create first";
    return DFTPAV_E_INVALID;
  }
  int first = 0, count = 0, block = 0;
  if (int rc = dftpav_comm_layout(global_B, h->comm_ranks, h->comm_rank, &first, &count, &block)) return rc;
  if (count != b->B) {
    h->err = "this batch is not the shard dftpav_comm_layout assigns to the rank";
    return DFTPAV_E_INVALID;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = finish_pending(b)) return rc;
  const size_t bytes = (size_t)block * 16;
  if (block <= b->B + 1) {
    // the send buffer IS the batch's record array (its epilogue-written records, one zero record of padding behind them for
    // the ranks whose shard is one short of the block): nothing of ours runs between the solve and the collective
    std::lock_guard<std::mutex> lk(h->comm_ref->mu);
    RCCLCHK(h, rccl().AllGather(b->d_records, all_records, bytes, kNcclUint8, h->comm, h->stream));
    return DFTPAV_OK;
  }
  if (h->comm_send_bytes < bytes) {
    if (h->d_comm_send) (void)hipFree(h->d_comm_send);
    h->d_comm_send = nullptr;
    HIPCHK(h, hipMalloc(&h->d_comm_send, bytes));
    h->comm_send_bytes = bytes;
  }
  HIPCHK(h, hipMemsetAsync(h->d_comm_send, 0, bytes, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_comm_send, b->d_records, (size_t)16 * count, hipMemcpyDeviceToDevice, h->stream));
  std::lock_guard<std::mutex> lk(h->comm_ref->mu);
  RCCLCHK(h, rccl().AllGather(h->d_comm_send, all_records, bytes, kNcclUint8, h->comm, h->stream));
  return DFTPAV_OK;
}
