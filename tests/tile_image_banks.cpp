// Host program of tests/test_cpu_tile_image_banks.py: the LDS bank multiplicities of the one tile image of the 64-query attention
// form (csn_amd/csrc/attn_tile_image.h), counted from the very offset functions the kernel calls.
// Rules (LDS banking per instruction): a bank is 4 bytes; stores bank on 32 dwords, ds_read_b64_tr_b16 and ds_read_b128 on 64;
// only lanes of one group conflict, equal addresses broadcast; the multiplicity of a group is the largest number of distinct
// dword addresses on one bank.
//   ds_write_b128:       8 groups of 8 consecutive lanes
//   ds_read_b64_tr_b16:  the two 32-lane halves
//   ds_read_b128:        {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32
// Prints "store S tr T row R mismatches M": the worst multiplicity of each access over every wave, piece / k-step / channel
// group, read and plane, and the number of (row, key, plane) elements on which the three accesses disagree or that are not
// reached exactly once by each.
#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <vector>

#include "attn_tile_image.h"

namespace ti = csn_tile_image;
constexpr int D = 256;

// lanes: (lane, first byte); width bytes per lane; banks: 32 or 64; groups: lane -> group id
static int worst(const std::vector<std::pair<int, int>>& lanes, int width, int banks, int (*group)(int)) {
  std::map<int, std::map<int, std::set<int>>> per;     // group -> bank -> distinct dword addresses
  for (auto [lane, a] : lanes)
    for (int b = 0; b < width; b += 4) per[group(lane)][((a + b) / 4) % banks].insert((a + b) / 4);
  int w = 0;
  for (auto& g : per)
    for (auto& b : g.second) w = std::max(w, (int)b.second.size());
  return w;
}
static int g_store(int l) { return l >> 3; }
static int g_tr(int l) { return l >> 5; }
static int g_row(int l) {
  const int m = l & 31;
  const bool first = m < 4 || (m >= 12 && m < 16) || (m >= 20 && m < 28);
  return 2 * (l >> 5) + (first ? 0 : 1);
}

int main() {
  int ws = 0, wt = 0, wr = 0, bad = 0;
  // what each access reaches: element -> times
  std::map<int, int> st_seen, tr_seen, rd_seen;
  for (int wave = 0; wave < 4; ++wave)
    for (int i = 0; i < 8; ++i) {
      std::vector<std::pair<int, int>> v;
      for (int l = 0; l < 64; ++l) {
        const int tid = 64 * wave + l, a = ti::store_off(D, tid, i);
        v.push_back({l, a});
        for (int k = 0; k < 8; ++k) {
          const int row = ti::store_row(tid, i), key = 8 * ti::store_unit(tid) + k, pl = ti::store_plane(tid);
          bad += a + 2 * k != ti::element(D, row, key, pl);
          ++st_seen[(pl * D + row) * ti::KT + key];
        }
      }
      ws = std::max(ws, worst(v, 16, 32, g_store));
    }
  for (int pl = 0; pl < 2; ++pl)
    for (int s = 0; s < D / 32; ++s)
      for (int h = 0; h < 2; ++h)
        for (int up = 0; up < 2; ++up) {
          std::vector<std::pair<int, int>> v;
          for (int l = 0; l < 64; ++l) {
            const int a = ti::tr_off(D, l, s, h, up, pl);
            v.push_back({l, a});
            bad += (a & 7) != 0;
            for (int k = 0; k < 4; ++k) {
              const int row = ti::tr_row(l, s, up), key = ti::tr_key(l, h) + k;
              bad += a + 2 * k != ti::element(D, row, key, pl);
              ++tr_seen[(pl * D + row) * ti::KT + key];
            }
          }
          wt = std::max(wt, worst(v, 8, 64, g_tr));
        }
  for (int pl = 0; pl < 2; ++pl)
    for (int c = 0; c < D / 16; ++c) {
      std::vector<std::pair<int, int>> v;
      for (int l = 0; l < 64; ++l) {
        const int a = ti::rd_off(D, l, c, pl);
        v.push_back({l, a});
        bad += (a & 15) != 0;
        for (int k = 0; k < 8; ++k) {
          const int row = ti::rd_row(l, c), key = 8 * (l >> 4) + k;
          bad += a + 2 * k != ti::element(D, row, key, pl);
          ++rd_seen[(pl * D + row) * ti::KT + key];
        }
      }
      wr = std::max(wr, worst(v, 16, 64, g_row));
    }
  // every element of both planes: stored once, read once by each read (a transposing read feeds 16 score rows: each element once)
  for (int e = 0; e < 2 * D * ti::KT; ++e) bad += st_seen[e] != 1 || tr_seen[e] != 1 || rd_seen[e] != 1;
  // the image stays inside its stage, planes do not overlap, and a lane's two accumulators together hold its 8 consecutive keys
  std::set<int> bytes;
  for (int pl = 0; pl < 2; ++pl)
    for (int row = 0; row < D; ++row)
      for (int key = 0; key < ti::KT; ++key) {
        const int a = ti::element(D, row, key, pl);
        bad += a < 0 || a + 2 > ti::stage_bytes(D) || !bytes.insert(a).second;
      }
  for (int l = 0; l < 64; ++l) {
    std::set<int> keys;
    for (int h = 0; h < 2; ++h)
      for (int r = 0; r < 4; ++r) {
        keys.insert(ti::acc_key(l, h, r));
        // accumulator row 4 kq + r was fed by the lanes of quarter p = kq: their keys tr_key .. + 3
        bad += ti::acc_key(l, h, r) != ti::tr_key(l >> 4, h) + r;
      }
    bad += keys.size() != 8 || *keys.begin() != 8 * (l >> 4) || *keys.rbegin() != 8 * (l >> 4) + 7;
  }
  std::printf("store %d tr %d row %d mismatches %d\n", ws, wt, wr, bad);
  return 0;
}
