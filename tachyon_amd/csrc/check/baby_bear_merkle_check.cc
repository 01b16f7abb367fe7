// Exercise include/tachyon_mi355x_merkle_tree.h the way a Tachyon build uses
// FieldMerkleTreeMMCS / TwoAdicFRI::Commit over BabyBear: Build on host
// matrices, GetRoot, digest_layers, an opening, and Commit (CosetLDEBatch on
// the device followed by the bit-reversed build on the holder's stream with
// no wait in between).  Only the two headers and the HIP runtime are used.
//   baby_bear_merkle_check [--external horizen|plonky3] [--gen <Montgomery word>] [--dump file] step...
//   step:  b<rows>x<cols>[,<rows>x<cols>...][r]   Build of seeded host matrices ('r': bit-reversed leaves)
//          c<L>x<cols>+<a>                        Commit of a 2^L x cols device matrix, log_blowup a, shift 31
//   --gen: the generator of order 2^LN as a Montgomery word, for 'c' steps (the
//          caller computes it; nothing comes from the library under test)
// dump, per step: the input matrices' words (for 'c' then the extension's), the
// layers from the leaf layer up, then the opening at index 1 (or 0 for a
// one-leaf tree): each matrix's row, then the siblings.  Prints one JSON line;
// exit 0 = every call returned true and the root equals the last layer.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tachyon_mi355x_merkle_tree.h"

namespace {

constexpr uint32_t kP = 0x78000001u;

struct BabyBear {
  uint32_t value;
};

struct Step {
  char kind = 'b';
  bool reversed = false;
  std::vector<std::pair<size_t, size_t>> dims;  // 'b': rows x cols; 'c': one entry, rows = 2^L
  unsigned added = 0;
};

bool number(const std::string& s, size_t* i, size_t* v) {
  const size_t start = *i;
  *v = 0;
  while (*i < s.size() && s[*i] >= '0' && s[*i] <= '9') *v = *v * 10 + (size_t)(s[(*i)++] - '0');
  return *i > start && *i - start < 10;
}

bool parse_step(const std::string& s, Step* st) {
  if (s.size() < 2 || (s[0] != 'b' && s[0] != 'c')) return false;
  st->kind = s[0];
  size_t i = 1;
  for (;;) {
    size_t r, c;
    if (!number(s, &i, &r) || i >= s.size() || s[i++] != 'x' || !number(s, &i, &c)) return false;
    st->dims.emplace_back(r, c);
    if (st->kind == 'b' && i < s.size() && s[i] == ',') {
      ++i;
      continue;
    }
    break;
  }
  if (st->kind == 'b') {
    if (i < s.size() && s[i] == 'r') st->reversed = true, ++i;
    return i == s.size();
  }
  size_t a;
  if (st->dims[0].first > 24 || i >= s.size() || s[i++] != '+' || !number(s, &i, &a) || a > 3) return false;
  st->dims[0].first = size_t(1) << st->dims[0].first;
  st->added = (unsigned)a;
  return i == s.size();
}

// seeded words in [0, p) (splitmix64; the dump carries them to the checker)
std::vector<BabyBear> seeded(uint64_t seed, size_t n) {
  std::vector<BabyBear> v(n);
  uint64_t x = seed;
  for (size_t i = 0; i < n; ++i) {
    x += 0x9e3779b97f4a7c15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    v[i].value = (uint32_t)(z % kP);
  }
  return v;
}

template <class T>
void put(FILE* f, const std::vector<T>& v) {
  if (f && !v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

}  // namespace

int main(int argc, char** argv) {
  namespace crypto = tachyon_mi355x;
  namespace math = tachyon_mi355x;
  using F = BabyBear;
  using Tree = crypto::FieldMerkleTree<F>;
  const char* dump = nullptr;
  crypto::Poseidon2ExternalMatrix external = crypto::Poseidon2ExternalMatrix::kHorizen;
  bool have_gen = false;
  F gen = {0};
  std::vector<Step> steps;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--dump" && i + 1 < argc) dump = argv[++i];
    else if (a == "--gen" && i + 1 < argc) gen.value = (uint32_t)strtoul(argv[++i], nullptr, 10), have_gen = true;
    else if (a == "--external" && i + 1 < argc && std::string(argv[i + 1]) == "horizen") ++i;
    else if (a == "--external" && i + 1 < argc && std::string(argv[i + 1]) == "plonky3")
      external = crypto::Poseidon2ExternalMatrix::kPlonky3, ++i;
    else {
      Step st;
      if (!parse_step(a, &st)) {
        fprintf(stderr, "baby_bear_merkle_check: bad argument '%s'\n", a.c_str());
        return 2;
      }
      if (st.kind == 'c' && !have_gen) {
        fprintf(stderr, "baby_bear_merkle_check: a 'c' step needs --gen before it\n");
        return 2;
      }
      steps.push_back(st);
    }
  }
  if (steps.empty()) {
    fprintf(stderr,
            "usage: baby_bear_merkle_check [--external horizen|plonky3] [--gen <Montgomery word>] [--dump file] step...\n");
    return 2;
  }

  FILE* f = dump ? fopen(dump, "wb") : nullptr;
  if (dump && !f) return 2;
  bool calls_ok = true, roots_ok = true;
  unsigned launches = 0;
  const F shift_mont = {(uint32_t)((31ULL << 32) % kP)};

  math::IcicleNTTHolder<F, math::kBabyBear> icicle_ntt_holder_;
  if (have_gen) {
    icicle_ntt_holder_ = math::IcicleNTTHolder<F, math::kBabyBear>::Create();
    math::IcicleNTTOptions options;
    options.are_inputs_on_device = options.are_outputs_on_device = true;
    options.is_async = true;
    calls_ok = icicle_ntt_holder_->Init(gen, options);
  }

  for (size_t s = 0; calls_ok && s < steps.size(); ++s) {
    const Step& st = steps[s];
    std::vector<std::vector<F>> inputs;
    for (size_t m = 0; m < st.dims.size(); ++m)
      inputs.push_back(seeded(0xB2B20000ULL + 16 * s + m, st.dims[m].first * st.dims[m].second));
    for (const auto& in : inputs) put(f, in);

    std::unique_ptr<Tree> tree;
    F* d_in = nullptr;
    F* d_out = nullptr;
    if (st.kind == 'b') {
      std::vector<crypto::MatrixView<F>> leaves;
      for (size_t m = 0; m < st.dims.size(); ++m)
        leaves.push_back({inputs[m].data(), st.dims[m].first, st.dims[m].second});
      tree = std::make_unique<Tree>(external);
      calls_ok = tree->Build(leaves, st.reversed);
    } else {
      const size_t rows = st.dims[0].first, cols = st.dims[0].second, out_rows = rows << st.added;
      if (hipMalloc(reinterpret_cast<void**>(&d_in), rows * cols * sizeof(F)) != hipSuccess ||
          hipMalloc(reinterpret_cast<void**>(&d_out), out_rows * cols * sizeof(F)) != hipSuccess ||
          hipMemcpy(d_in, inputs[0].data(), rows * cols * sizeof(F), hipMemcpyHostToDevice) != hipSuccess)
        return 2;
      tree = crypto::Commit<F>(icicle_ntt_holder_, {{d_in, rows, cols}}, st.added, shift_mont, {d_out}, external);
      calls_ok = tree != nullptr;
      if (calls_ok) {
        // the root first: it waits for the stream the extension and the build were enqueued on
        const Tree::Digest root = tree->GetRoot();
        (void)root;
        std::vector<F> lde(out_rows * cols);
        if (hipMemcpy(lde.data(), d_out, lde.size() * sizeof(F), hipMemcpyDeviceToHost) != hipSuccess) return 2;
        put(f, lde);
      }
    }
    if (calls_ok) {
      const Tree::Digest root = tree->GetRoot();
      const std::vector<std::vector<Tree::Digest>> layers = tree->digest_layers();
      roots_ok = roots_ok && !layers.empty() && layers.back().size() == 1 &&
                 memcmp(&layers.back()[0], &root, sizeof(root)) == 0;
      for (const auto& layer : layers) put(f, layer);
      std::vector<std::vector<F>> openings;
      std::vector<Tree::Digest> proof;
      calls_ok = tree->CreateOpeningProof(layers.size() > 1 ? 1 : 0, &openings, &proof);
      calls_ok = calls_ok && proof.size() + 1 == layers.size() && openings.size() == st.dims.size();
      for (const auto& row : openings) put(f, row);
      put(f, proof);
      launches = tree->last_launches();
    }
    tree.reset();
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
  }
  if (f) fclose(f);
  printf("{\"field\": \"baby_bear\", \"external\": \"%s\", \"steps\": %zu, \"calls\": %s, \"roots\": %s, "
         "\"last_launches\": %u}\n",
         external == crypto::Poseidon2ExternalMatrix::kHorizen ? "horizen" : "plonky3", steps.size(),
         calls_ok ? "true" : "false", roots_ok ? "true" : "false", launches);
  return calls_ok && roots_ok ? 0 : 1;
}
