// C-ABI of the DuplexChallenger, its grind, the batched openings and the
// opening proof in one call (include/tachyon_mi355x.h): int results, nothing
// aborts across this boundary.  The challenger's entry points are host code and
// work without a GPU.
#include "../../../include/tachyon_mi355x.h"

#include <cstring>
#include <memory>
#include <vector>

#include "../common/hip_util.h"
#include "../fri/grind_bb.h"
#include "capi_handles.h"
#include "merkle_tree_validate.h"

using namespace tachyon_amd;
using Challenger = tachyon_mi355x_baby_bear_duplex_challenger;
using FriProof = tachyon_mi355x_baby_bear_fri_proof;

static_assert(fri::kChallengerStateWords == 50);

extern "C" {

Challenger* tachyon_mi355x_baby_bear_duplex_challenger_create(int external_matrix, unsigned rate) {
  if (!merkle_tree::external_ok(external_matrix) || !fri::challenger_rate_ok(rate)) return nullptr;
  return guarded<Challenger*>(
      nullptr, [&] { return new Challenger{fri::DuplexChallenger(external_matrix, rate), nullptr}; });
}

Challenger* tachyon_mi355x_baby_bear_duplex_challenger_clone(const Challenger* c) {
  if (!c) return nullptr;
  return guarded<Challenger*>(nullptr, [&] { return new Challenger{c->challenger, nullptr}; });
}

void tachyon_mi355x_baby_bear_duplex_challenger_destroy(Challenger* c) {
  try {
    delete c;
  } catch (...) {
  }
}

int tachyon_mi355x_baby_bear_duplex_challenger_observe(Challenger* c, const uint32_t* values, size_t count) {
  if (!c || (!values && count)) return 0;
  return c->challenger.observe(values, count) ? 1 : 0;
}

int tachyon_mi355x_baby_bear_duplex_challenger_sample(Challenger* c, uint32_t* out, size_t count) {
  if (!c || !out) return 0;
  for (size_t i = 0; i < count; ++i) out[i] = c->challenger.sample();
  return 1;
}

int tachyon_mi355x_baby_bear_duplex_challenger_sample_ext(Challenger* c, void* out) {
  if (!c || !out) return 0;
  uint32_t e[4];
  c->challenger.sample_ext(e);
  memcpy(out, e, sizeof e);
  return 1;
}

int tachyon_mi355x_baby_bear_duplex_challenger_sample_bits(Challenger* c, unsigned bits, uint32_t* out) {
  if (!c || !out || bits > fri::kMaxSampleBits) return 0;
  *out = c->challenger.sample_bits(bits);
  return 1;
}

int tachyon_mi355x_baby_bear_duplex_challenger_check_witness(Challenger* c, unsigned bits, uint32_t witness) {
  if (!c || bits > fri::kMaxSampleBits || witness >= bb31::kP) return 0;
  return c->challenger.check_witness(bits, witness) ? 1 : 0;
}

int tachyon_mi355x_baby_bear_duplex_challenger_state(const Challenger* c, uint32_t* out) {
  if (!c || !out) return 0;
  c->challenger.dump(out);
  return 1;
}

int tachyon_mi355x_baby_bear_duplex_challenger_grind_range(Challenger* c, unsigned bits, uint64_t from, uint64_t to,
                                                           uint32_t* witness_out, void* stream) {
  if (!c || !witness_out || !fri::grind_args_ok(bits, from, to)) return 0;
  return guarded(0, [&] {
    require_gpu();
    if (!c->grind) c->grind = std::make_unique<DeviceBuffer>();
    return fri::grind(c->challenger, bits, from, to, witness_out, *c->grind, static_cast<hipStream_t>(stream));
  });
}

int tachyon_mi355x_baby_bear_duplex_challenger_grind(Challenger* c, unsigned bits, uint32_t* witness_out,
                                                     void* stream) {
  return tachyon_mi355x_baby_bear_duplex_challenger_grind_range(c, bits, 0, bb31::kP, witness_out, stream);
}

int tachyon_mi355x_baby_bear_merkle_tree_open_batch(tachyon_mi355x_baby_bear_merkle_tree* tree, const size_t* indices,
                                                    size_t count, void* const* rows_out, void* siblings_out) {
  if (!tree || !indices || !rows_out) return 0;
  return guarded(0, [&] { return tree->tree->open_batch(indices, count, rows_out, siblings_out); });
}

int tachyon_mi355x_baby_bear_fri_opening_answer_queries(tachyon_mi355x_baby_bear_fri_opening* h, const size_t* indices,
                                                        size_t count, void* sibling_values_out, void* siblings_out) {
  if (!h || !indices) return 0;
  return guarded(0, [&] { return h->fri->answer_queries(indices, count, sibling_values_out, siblings_out); });
}

FriProof* tachyon_mi355x_baby_bear_fri_opening_prove(tachyon_mi355x_baby_bear_fri_opening* h, Challenger* challenger,
                                                     const tachyon_mi355x_baby_bear_fri_round* rounds,
                                                     size_t num_rounds, size_t num_queries,
                                                     unsigned proof_of_work_bits) {
  if (!h || !challenger || !rounds || num_rounds == 0) return nullptr;
  return guarded<FriProof*>(nullptr, [&]() -> FriProof* {
    std::vector<fri::ProveRound> rs(num_rounds);
    for (size_t r = 0; r < num_rounds; ++r) {
      if (!rounds[r].tree) return nullptr;
      rs[r] = fri::ProveRound{rounds[r].tree->tree.get(), rounds[r].points, rounds[r].num_points,
                              rounds[r].opened_values_out};
    }
    auto proof = std::make_unique<FriProof>();
    if (!h->fri->prove(challenger->challenger, rs.data(), num_rounds, num_queries, proof_of_work_bits, &proof->proof))
      return nullptr;
    return proof.release();
  });
}

void tachyon_mi355x_baby_bear_fri_proof_destroy(FriProof* proof) {
  try {
    delete proof;
  } catch (...) {
  }
}

size_t tachyon_mi355x_baby_bear_fri_proof_num_commits(const FriProof* proof) {
  return proof ? proof->proof.num_commits() : 0;
}

int tachyon_mi355x_baby_bear_fri_proof_commits(const FriProof* proof, void* out) {
  if (!proof || !out) return 0;
  memcpy(out, proof->proof.commits.data(), proof->proof.commits.size() * sizeof(uint32_t));
  return 1;
}

int tachyon_mi355x_baby_bear_fri_proof_final_eval(const FriProof* proof, void* out) {
  if (!proof || !out) return 0;
  memcpy(out, proof->proof.final_eval.c, 4 * sizeof(uint32_t));
  return 1;
}

int tachyon_mi355x_baby_bear_fri_proof_pow_witness(const FriProof* proof, uint32_t* out) {
  if (!proof || !out) return 0;
  *out = proof->proof.pow_witness;
  return 1;
}

size_t tachyon_mi355x_baby_bear_fri_proof_num_queries(const FriProof* proof) {
  return proof ? proof->proof.indices.size() : 0;
}

size_t tachyon_mi355x_baby_bear_fri_proof_query_index(const FriProof* proof, size_t q) {
  return proof && q < proof->proof.indices.size() ? proof->proof.indices[q] : 0;
}

int tachyon_mi355x_baby_bear_fri_proof_query_steps(const FriProof* proof, size_t q, void* sibling_values_out,
                                                   void* siblings_out) {
  if (!proof || q >= proof->proof.indices.size()) return 0;
  const fri::Proof& p = proof->proof;
  const size_t commits = p.num_commits();
  if (commits == 0) return 1;  // nothing was committed: nothing to copy
  const size_t total = fri::query_total_siblings(p.log_max, (unsigned)commits);
  if (!sibling_values_out || (total && !siblings_out)) return 0;
  memcpy(sibling_values_out, p.sibling_values.data() + q * commits * 4, commits * 4 * sizeof(uint32_t));
  if (total) memcpy(siblings_out, p.siblings.data() + q * total * 8, total * 8 * sizeof(uint32_t));
  return 1;
}

int tachyon_mi355x_baby_bear_fri_proof_query_input(const FriProof* proof, size_t q, size_t round,
                                                   void* const* rows_out, void* siblings_out) {
  if (!proof || !rows_out || q >= proof->proof.indices.size() || round >= proof->proof.rounds.size()) return 0;
  const fri::Proof::RoundOpenings& ro = proof->proof.rounds[round];
  if (ro.num_siblings && !siblings_out) return 0;
  for (size_t m = 0; m < ro.cols.size(); ++m)
    if (!rows_out[m]) return 0;
  for (size_t m = 0; m < ro.cols.size(); ++m)
    memcpy(rows_out[m], ro.rows[m].data() + q * ro.cols[m], ro.cols[m] * sizeof(uint32_t));
  if (ro.num_siblings)
    memcpy(siblings_out, ro.siblings.data() + q * ro.num_siblings * 8, ro.num_siblings * 8 * sizeof(uint32_t));
  return 1;
}

}  // extern "C"
