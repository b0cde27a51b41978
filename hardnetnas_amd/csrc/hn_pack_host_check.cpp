// Host-only run of hn_pack.h's weight packers -- the index arithmetic that writes the kernels' device layouts -- at
// every shape hn_create's build_hardnet, build_nas, build_fdl and build_nas_layers (hn_api.hip) pass them: the stock
// HardNet, every arch.MODEL_ARCH name, both FDL variants, and each of the 17 candidate ops at each of the six
// SEARCH_SPACE2 layers, deduplicated by (packer, shape).  Weights come from a fixed LCG seeded by the pair's name.
// Checked for each pair:
//   - the sanitizers are silent (no read outside the weights, no write outside the output);
//   - the output has the size the layout comment states, and a packer that advances a write cursor has reached the
//     end of what it allocated (its last fragment is written: not all zero);
//   - no weight left the fp16 range (put_f16_split's counter);
//   - a 64-bit FNV-1a digest of the output bytes equals the line `packer shape digest` of the file given as argument
//     (tests/golden/pack_digests.txt, recorded from the packers before they moved into hn_pack.h).
// `--print` writes the table instead of comparing.  Built by `make pack_check` with -DHN_EXPERIMENTS (pack_wino too)
// and the address and undefined-behaviour sanitizers.  Stand-alone: links nothing of the library, needs no GPU.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

#include "hn_pack.h"

namespace packcheck {

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::fprintf(stderr, "FAILED %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);          \
      std::fprintf(stderr, "\n");                 \
      std::exit(1);                               \
    }                                             \
  } while (0)

constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;
template <class T>
uint64_t fnv1a(const std::vector<T>& v, uint64_t h = kFnvBasis) {
  const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * kFnvPrime;
  return h;
}

std::map<std::string, uint64_t> g_done;  // "packer shape" -> digest

// n weights in [-1, 1) from a 64-bit LCG seeded by the pair's name
std::vector<float> weights(const std::string& key, size_t n) {
  uint64_t s = kFnvBasis;
  for (unsigned char c : key) s = (s ^ c) * kFnvPrime;
  std::vector<float> w(n);
  for (float& x : w) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    x = (float)((double)(s >> 40) / (double)(1 << 23) - 1.0);
  }
  return w;
}

// one (packer, shape): run(w) packs the n_in weights and returns the digest after checking the output's size
template <class Run>
void pair(const std::string& packer, const std::string& shape, size_t n_in, Run run) {
  const std::string key = packer + " " + shape;
  if (g_done.count(key)) return;
  tl_f16_out_of_range = 0;
  g_done[key] = run(weights(key, n_in));
  CHECK(tl_f16_out_of_range == 0, "%s: %ld weights outside the fp16 range", key.c_str(), tl_f16_out_of_range);
}

// size as the layout states it; cursor: the packer advances `o` by fragments of 2 x 64 x 8 and must end at the size
template <class T>
uint64_t sized(const char* what, const std::vector<T>& out, size_t want, bool cursor = false) {
  CHECK(out.size() == want, "%s: %zu elements, the layout has %zu", what, out.size(), want);
  if (cursor) {
    bool written = false;
    for (size_t i = want - 2 * 64 * 8; i < want; ++i) written |= out[i] != 0;
    CHECK(written, "%s: the write cursor stopped before the end of the output", what);
  }
  return fnv1a(out);
}

std::string shp(std::initializer_list<int> v) {
  std::ostringstream s;
  for (int x : v) s << (s.tellp() ? "," : "") << x;
  return s.str();
}

constexpr size_t kFrag = 2 * 64 * 8;  // hi + lo planes of one 64-lane fragment

void conv3x3(int cin, int cout) {
  pair("pack_conv3x3", shp({cin, cout}), (size_t)cout * cin * 9, [&](const std::vector<float>& w) {
    return sized("pack_conv3x3", pack_conv3x3(w, cin, cout), (size_t)(cin / 32) * 9 * 2 * (cout / 32) * kFrag, true);
  });
}
void head(int cin, int kk, bool f16) {
  pair("pack_head", shp({cin, kk, f16}), (size_t)128 * cin * kk * kk, [&](const std::vector<float>& w) {
    return sized("pack_head", pack_head(w, cin, kk, f16), (size_t)(cin * kk * kk / 16) * 4 * kFrag, true);
  });
}
void wino1(int cin, int cout) {
  pair("pack_wino1", shp({cin, cout}), (size_t)cout * cin * 9, [&](const std::vector<float>& w) {
    return sized("pack_wino1", pack_wino1(w, cin, cout), (size_t)(cin / 32) * 24 * (cout / 32) * kFrag, true);
  });
}
void wino4(int cin, int cout) {
  pair("pack_wino4", shp({cin, cout}), (size_t)cout * cin * 9, [&](const std::vector<float>& w) {
    return sized("pack_wino4", pack_wino4(w, cin, cout), (size_t)(cin / 32) * 18 * (cout / 16) * kFrag, true);
  });
}
#ifdef HN_EXPERIMENTS
void wino(int cin, int cout) {
  pair("pack_wino", shp({cin, cout}), (size_t)cout * cin * 9, [&](const std::vector<float>& w) {
    return sized("pack_wino", pack_wino(w, cin, cout), (size_t)(cout / 32) * (cin / 16) * 16 * kFrag);
  });
}
#endif
void c12(int cout) {
  pair("pack_c12", shp({cout}), (size_t)cout * 32 * 9, [&](const std::vector<float>& w) {
    return sized("pack_c12", pack_c12(w, cout), (size_t)9 * (cout / 16) * kFrag);
  });
}
void c12w() {
  pair("pack_c12w", "-", (size_t)32 * 32 * 9, [&](const std::vector<float>& w) {
    return sized("pack_c12w", pack_c12w(w), (size_t)6 * 3 * 2 * kFrag);
  });
}
void taps() {
  pair("stem_taps", "-", 32 * 9, [&](const std::vector<float>& w) { return sized("stem_taps", stem_taps(w), 9 * 32); });
}
void front_stem() {
  pair("pack_front_stem", "-", 32 * 9, [&](const std::vector<float>& w) {
    return sized("pack_front_stem", pack_front_stem(Folded{w, {}}), 2 * kFrag);
  });
}
void transpose(int cout, int kg) {
  pair("transpose_pw", shp({cout, kg}), (size_t)cout * kg, [&](const std::vector<float>& w) {
    return sized("transpose_pw", transpose_pw(w, cout, kg), (size_t)kg * cout);
  });
}
void front(int mid, int g) {  // Folded: [mid][32 / g] weights, then the mid biases
  const size_t nw = (size_t)mid * (32 / g);
  pair("pack_front", shp({mid, g}), nw + mid, [&](const std::vector<float>& w) {
    std::vector<uint16_t> a;
    std::vector<float> b;
    pack_front(Folded{{w.begin(), w.begin() + nw}, {w.begin() + nw, w.end()}}, mid, g, &a, &b);
    sized("pack_front bias", b, mid);
    return fnv1a(b, sized("pack_front", a, (size_t)(mid / 32) * 2 * kFrag));
  });
}
// shuffle: rows in ChannelShuffle(g) order (build_nas_layers' src), else as they are
void a1x1(int cout, int cin, int g, bool shuffle) {
  pair("pack_1x1_a", shp({cout, cin, g, shuffle}), (size_t)cout * (cin / g), [&](const std::vector<float>& w) {
    const int cg = cout / g;
    auto src = [&](int d) { return shuffle && g > 1 ? (d % g) * cg + d / g : d; };
    return sized("pack_1x1_a", pack_1x1_a(w, cout, cin, g, src), (size_t)(cout / 32) * (cin / 16) * kFrag);
  });
}
void a1x1_16(int cout, int cin, int g) {
  pair("pack_1x1_a16", shp({cout, cin, g}), (size_t)cout * (cin / g), [&](const std::vector<float>& w) {
    return sized("pack_1x1_a16", pack_1x1_a16(w, cout, cin, g), (size_t)(cin / 32) * (cout / 16) * kFrag);
  });
}

// build_hardnet's calls
void hardnet() {
  static const int cin[7] = {1, 32, 32, 64, 64, 128, 128}, cout[7] = {32, 32, 64, 64, 128, 128, 128};
  for (int l = 1; l < 7; ++l) {
    if (l < 6) conv3x3(cin[l], cout[l]);
    else head(128, 8, false);
    if (l == 3 || l == 5) wino1(cin[l], cout[l]);
    if (l == 3) wino4(cin[l], cout[l]);  // (called by the experiments library only, as pack_wino)
#ifdef HN_EXPERIMENTS
    if (l == 3 || l == 5) wino(cin[l], cout[l]);
#endif
    if (l == 1 || l == 2) c12(cout[l]);
    if (l == 1) c12w();
  }
}

// the candidate ops (hn_api.hip kHnOps: skip, expansion, kernel, pw groups), SEARCH_SPACE2 and the named models
struct Op {
  int skip, e, k, g;
};
const Op kCand[17] = {{1, 0, 0, 0}, {0, 1, 3, 1}, {0, 3, 3, 1}, {0, 4, 3, 4}, {0, 1, 5, 1}, {0, 3, 5, 1},
                      {0, 4, 5, 4}, {0, 1, 3, 1}, {0, 3, 3, 1}, {0, 4, 3, 4}, {0, 1, 5, 1}, {0, 3, 5, 1},
                      {0, 4, 5, 4}, {0, 1, 3, 2}, {0, 1, 5, 2}, {0, 1, 3, 2}, {0, 1, 5, 2}};
struct Layer {
  int cin, cout, stride;
};
const Layer kSpace[6] = {{32, 32, 2}, {32, 32, 1}, {32, 64, 2}, {64, 64, 1}, {64, 128, 2}, {128, 128, 1}};
const Layer kFdlLayers[3] = {{64, 64, 1}, {64, 128, 2}, {128, 128, 1}};
const int kFdlOps[3] = {4, 2, 14};
const int kModels[3][6] = {{1, 4, 14, 13, 4, 0}, {4, 0, 4, 0, 0, 0}, {0, 0, 14, 13, 4, 4}};  // wang2, wang3, wang4

// build_nas_layers' calls for layer i.  Every block of these spaces has a fused kernel (hn_front_supported for
// layer 0 of a NAS model, hn_irf_supported for the others and for FDL), so the fused operands are always packed.
void nas_layer(int i, const Layer& L, const Op& s, bool fdl) {
  if (s.skip) {
    if (L.cin != L.cout) {
      transpose(L.cout, L.cin);
      if (L.cin == 64 && L.cout == 128) a1x1(L.cout, L.cin, 1, false);
    }
    return;
  }
  const int mid = L.cin * s.e;
  const bool is_front = i == 0 && !fdl;
  transpose(mid, L.cin / s.g);
  if (is_front) front(mid, s.g);
  else a1x1(mid, L.cin, s.g, true);
  transpose(L.cout, mid / s.g);
  a1x1(L.cout, mid, s.g, false);
  if (is_front) a1x1_16(L.cout, mid, s.g);
}
void nas_model(const int* ops) {  // build_nas
  taps();
  front_stem();
  for (int i = 0; i < 6; ++i) nas_layer(i, kSpace[i], kCand[ops[i]], false);
  head(128, 4, true);
}
void fdl_model(bool v0) {  // build_fdl
  taps();
  if (v0) transpose(32, 32);
  transpose(64, 32);
  for (int i = 0; i < 3; ++i) nas_layer(i, kFdlLayers[i], kCand[kFdlOps[i]], true);
  head(128, 4, true);
}

}  // namespace packcheck

int main(int argc, char** argv) {
  using namespace packcheck;
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s tests/golden/pack_digests.txt | --print\n", argv[0]);
    return 2;
  }
  hardnet();
  for (const auto& ops : kModels) nas_model(ops);
  fdl_model(true);
  fdl_model(false);
  for (int i = 0; i < 6; ++i)
    for (int op = 0; op < 17; ++op) nas_layer(i, kSpace[i], kCand[op], false);
  if (std::string(argv[1]) == "--print") {
    for (const auto& kv : g_done) std::printf("%s %016" PRIx64 "\n", kv.first.c_str(), kv.second);
    return 0;
  }
  std::ifstream f(argv[1]);
  CHECK(f.good(), "cannot read %s", argv[1]);
  std::map<std::string, uint64_t> golden;
  for (std::string line; std::getline(f, line);) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream s(line);
    std::string packer, shape, digest;
    CHECK(bool(s >> packer >> shape >> digest), "%s: malformed line '%s'", argv[1], line.c_str());
    golden[packer + " " + shape] = std::strtoull(digest.c_str(), nullptr, 16);
  }
  for (const auto& kv : g_done) {
    CHECK(golden.count(kv.first), "%s has no line for '%s'", argv[1], kv.first.c_str());
    CHECK(golden[kv.first] == kv.second, "%s: digest %016" PRIx64 ", recorded %016" PRIx64, kv.first.c_str(), kv.second,
          golden[kv.first]);
  }
  CHECK(golden.size() == g_done.size(), "%s has %zu lines, the packers are called at %zu shapes", argv[1], golden.size(),
        g_done.size());
  std::printf("pack_check: %zu (packer, shape) pairs, sizes and digests match\n", g_done.size());
  return 0;
}
