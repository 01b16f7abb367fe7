// The opaque handles of the BabyBear entry points that more than one capi_*.hip
// file takes (include/tachyon_mi355x.h declares them); their entry points run
// under guarded() (capi_guard.h).
#pragma once
#include <memory>

#include "../fri/challenger_bb.h"
#include "../fri/fri_bb.h"
#include "../hash/merkle_bb.h"
#include "capi_guard.h"

struct tachyon_mi355x_baby_bear_merkle_tree {
  std::unique_ptr<tachyon_amd::hash::BbMerkleTree> tree;
};

struct tachyon_mi355x_baby_bear_fri_opening {
  std::unique_ptr<tachyon_amd::fri::FriOpening> fri;
};

// the transcript is host state; the device word of its grind is allocated by the first _grind
struct tachyon_mi355x_baby_bear_duplex_challenger {
  tachyon_amd::fri::DuplexChallenger challenger;
  std::unique_ptr<tachyon_amd::DeviceBuffer> grind;
};

struct tachyon_mi355x_baby_bear_fri_proof {
  tachyon_amd::fri::Proof proof;
};
