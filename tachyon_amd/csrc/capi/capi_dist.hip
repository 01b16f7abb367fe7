// C-ABI of the multi-process layer (include/tachyon_mi355x.h): the BN254
// four-step NTT plan of one rank and the communicators (dist/comm.h).  The
// sharded MSM entry points that take a communicator are in capi_msm.hip.
#include "../../../include/tachyon_mi355x.h"

#include <cstring>
#include <memory>

#include "../dist/comm.h"
#include "../ntt/ntt.h"
#include "capi_guard.h"

using namespace tachyon_amd;

struct tachyon_mi355x_bn254_ntt4 {
  ntt::Ntt4Step<Bn254Fr>* impl;
  DeviceBuffer send, recv;  // tachyon_mi355x_bn254_ntt4_run's exchange buffers
};

extern "C" {

tachyon_mi355x_bn254_ntt4* tachyon_mi355x_bn254_ntt4_create(uint32_t log_n, uint32_t log_world, uint32_t rank,
                                                           void* stream) {
  GUARD_BEGIN
  return new tachyon_mi355x_bn254_ntt4{
      new ntt::Ntt4Step<Bn254Fr>(log_n, log_world, rank, static_cast<hipStream_t>(stream))};
  GUARD_END
}
tachyon_mi355x_bn254_ntt4* tachyon_mi355x_bn254_ntt4_create_split(uint32_t log_n, uint32_t log_r, uint32_t log_world,
                                                                 uint32_t rank, void* stream) {
  GUARD_BEGIN
  if (log_r == 0 || log_r >= log_n) throw std::runtime_error("tachyon_mi355x: ntt4 split needs 1 <= log_r < log_n");
  return new tachyon_mi355x_bn254_ntt4{
      new ntt::Ntt4Step<Bn254Fr>(log_n, log_world, rank, static_cast<hipStream_t>(stream), log_r)};
  GUARD_END
}
uint32_t tachyon_mi355x_bn254_ntt4_log_rows(const tachyon_mi355x_bn254_ntt4* plan) { return plan->impl->log_rows(); }
uint32_t tachyon_mi355x_ntt4_split_log_r(uint32_t log_n, uint32_t log_world) {
  return ntt::ntt4_split_log_r(log_n, log_world);
}
void tachyon_mi355x_bn254_ntt4_destroy(tachyon_mi355x_bn254_ntt4* plan) {
  if (!plan) return;
  delete plan->impl;
  delete plan;
}
size_t tachyon_mi355x_bn254_ntt4_local_size(const tachyon_mi355x_bn254_ntt4* plan) { return plan->impl->local_size(); }
void tachyon_mi355x_bn254_ntt4_stage(tachyon_mi355x_bn254_ntt4* plan, int stage, int inverse,
                                     const tachyon_bn254_fr* d_in, tachyon_bn254_fr* d_out) {
  GUARD_BEGIN
  const Bn254Fr* in = reinterpret_cast<const Bn254Fr*>(d_in);
  Bn254Fr* out = reinterpret_cast<Bn254Fr*>(d_out);
  if (stage != 1 && stage != 2) throw std::runtime_error("tachyon_mi355x: ntt4 stage is 1 or 2");
  if (!inverse) (stage == 1) ? plan->impl->forward_stage1(in, out) : plan->impl->forward_stage2(in, out);
  else (stage == 1) ? plan->impl->inverse_stage1(in, out) : plan->impl->inverse_stage2(in, out);
  GUARD_END
}
// Both stages and the all-to-all between them, on the plan's stream (RCCL:
// no host synchronisation; the host-staged communicator synchronises it)
void tachyon_mi355x_bn254_ntt4_run(tachyon_mi355x_bn254_ntt4* plan, tachyon_mi355x_comm* comm, int inverse,
                                   const tachyon_bn254_fr* d_in, tachyon_bn254_fr* d_out) {
  GUARD_BEGIN
  if (!comm || !comm->impl) throw std::runtime_error("null communicator");
  auto& p = *plan->impl;
  if ((uint32_t)comm->impl->world() != p.world() || (uint32_t)comm->impl->rank() != p.rank())
    throw std::runtime_error("tachyon_mi355x: ntt4 plan world/rank differ from the communicator's");
  const size_t bytes = p.local_size() * sizeof(Bn254Fr);
  Bn254Fr* send = static_cast<Bn254Fr*>(plan->send.ensure(bytes));
  Bn254Fr* recv = static_cast<Bn254Fr*>(plan->recv.ensure(bytes));
  const Bn254Fr* in = reinterpret_cast<const Bn254Fr*>(d_in);
  Bn254Fr* out = reinterpret_cast<Bn254Fr*>(d_out);
  if (!inverse) p.forward_stage1(in, send);
  else p.inverse_stage1(in, send);
  comm->impl->all_to_all_device(send, recv, bytes / p.world(), p.stream());
  if (!inverse) p.forward_stage2(recv, out);
  else p.inverse_stage2(recv, out);
  GUARD_END
}
int tachyon_mi355x_bn254_ntt4_set_variant(tachyon_mi355x_bn254_ntt4* plan, int variant) {
  if (variant < 0 || variant > 15) return 0;
  GUARD_BEGIN plan->impl->set_variant(variant); GUARD_END
  return 1;
}
void* tachyon_mi355x_bn254_ntt4_stream(const tachyon_mi355x_bn254_ntt4* plan) {
  return static_cast<void*>(plan->impl->stream());
}
void tachyon_mi355x_bn254_ntt4_synchronize(tachyon_mi355x_bn254_ntt4* plan) {
  GUARD_BEGIN
  TA_HIP(hipStreamSynchronize(plan->impl->stream()));
  GUARD_END
}

// ---- communicators (dist/comm.h) ----
int tachyon_mi355x_comm_unique_id(void* out, size_t cap) {
  if (cap < sizeof(ncclUniqueId)) return 0;
  GUARD_BEGIN
  const ncclUniqueId id = dist::rccl_unique_id();
  memcpy(out, &id, sizeof(id));
  return (int)sizeof(id);
  GUARD_END
  return 0;
}
tachyon_mi355x_comm* tachyon_mi355x_comm_init_rccl(const void* unique_id, int world, int rank) {
  GUARD_BEGIN
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof(id));
  auto* c = new tachyon_mi355x_comm();
  c->impl = std::make_unique<dist::RcclComm>(id, world, rank);
  return c;
  GUARD_END
  return nullptr;
}
tachyon_mi355x_comm* tachyon_mi355x_comm_from_rccl(void* nccl_comm) {
  GUARD_BEGIN
  auto* c = new tachyon_mi355x_comm();
  c->impl = std::make_unique<dist::RcclComm>(static_cast<ncclComm_t>(nccl_comm));
  return c;
  GUARD_END
  return nullptr;
}
tachyon_mi355x_comm* tachyon_mi355x_comm_create_host(int world, int rank, tachyon_mi355x_all_gather_fn all_gather,
                                                     tachyon_mi355x_all_to_all_fn all_to_all, void* user) {
  GUARD_BEGIN
  auto* c = new tachyon_mi355x_comm();
  c->impl = std::make_unique<dist::HostComm>(world, rank, all_gather, all_to_all, user);
  return c;
  GUARD_END
  return nullptr;
}
void tachyon_mi355x_comm_destroy(tachyon_mi355x_comm* comm) { delete comm; }
void tachyon_mi355x_comm_all_gather(tachyon_mi355x_comm* comm, const void* send, void* recv, size_t bytes) {
  GUARD_BEGIN comm->impl->all_gather_host(send, recv, bytes); GUARD_END
}
int tachyon_mi355x_comm_world(const tachyon_mi355x_comm* comm) { return comm->impl->world(); }
int tachyon_mi355x_comm_rank(const tachyon_mi355x_comm* comm) { return comm->impl->rank(); }
const char* tachyon_mi355x_comm_backend(const tachyon_mi355x_comm* comm) { return comm->impl->backend(); }

}  // extern "C"
