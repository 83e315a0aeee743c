// The ONE LDS image of a [d][32 keys] bf16 hi / lo tile that the 64-query form of the d = 256 attention kernels (attn_bf16x3.hip,
// WG64) fills once and reads twice: phase 1 with the transposing read (ds_read_b64_tr_b16, 8 bytes = 4 keys of a row per lane),
// phase 2 with the row read (ds_read_b128, 16 bytes = 8 keys of a row per lane).  Plain constexpr functions of integers, so that
// host code (tests/test_cpu_tile_image_banks.py) enumerates exactly the addresses the kernel forms.
//
// Image: a row is its 64 natural bytes per plane; the 16-byte unit u (keys 8 u .. 8 u + 7, in order) of row r sits at unit
// u ^ X(r), X = {0, 2, 3, 1}[(r >> 2) & 3]; the lo plane starts 64 bytes out of phase (plane pitch = D * 64 + 64 bytes).
//   staging store (ds_write_b128, 8-lane groups, 32 banks): a group is one row, 4 hi + 4 lo units = 128 bytes, the planes on
//     complementary halves — 1-way;
//   row read (4 groups of 16 lanes, 64 banks): a group holds rows {0-3, 12-15} at unit kq and {4-11} at unit kq ^ 1; per row & 3
//     the four units {X0, X3, 1 ^ X1, 1 ^ X2} = {0, 1, 2, 3} resp. {X1, X2, 1 ^ X0, 1 ^ X3} = {2, 3, 1, 0} — 1-way;
//   transposing read (2 groups of 32 lanes, 64 banks): a group takes rows r .. r + 3 and r + 8 .. r + 11, all four units of each;
//     units stay whole (the row read needs them in order), so the two rows 8 apart can only part by their 8-byte HALF: the
//     16-lane quarter p of a group (score rows 4 p .. 4 p + 3) reads half h ^ (p & 1) in read h — S0 row i is key
//     8 (i >> 2) + 4 ((i >> 2) & 1) + (i & 3) and S1 the other half, which a lane undoes by renaming its two accumulators when
//     its quarter is odd — and X(r + 8) = X(r) ^ 3 sends the even units of one row where the odd units of the other are: 1-way.
#pragma once

namespace csn_tile_image {

constexpr int KT = 32;                                             // keys per tile
constexpr int ROW_B = 2 * KT;                                      // bytes of a row in one plane
constexpr int plane_bytes(int d) { return d * ROW_B + 64; }        // hi -> lo: 64 bytes out of phase
constexpr int stage_bytes(int d) { return 2 * plane_bytes(d); }
constexpr int unit_xor(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }   // {0, 2, 3, 1}

// byte offset of element (row, key) of a plane from the stage's base — what all three accesses must agree on
constexpr int element(int d, int row, int key, int plane) {
  return plane * plane_bytes(d) + row * ROW_B + 16 * ((key >> 3) ^ unit_xor(row)) + 2 * (key & 7);
}

// staging store: thread tid of 256 holds, as piece i (0..7), the 16-byte unit tid & 3 of plane (tid >> 2) & 1 of row (tid >> 3) + 32 i
constexpr int store_row(int tid, int i) { return (tid >> 3) + 32 * i; }
constexpr int store_unit(int tid) { return tid & 3; }
constexpr int store_plane(int tid) { return (tid >> 2) & 1; }
constexpr int store_off(int d, int tid, int i) { return element(d, store_row(tid, i), 8 * store_unit(tid), store_plane(tid)); }

// transposing read h (0 / 1: accumulator S0 / S1) of k-step s (rows 32 s ..), upper (0) or lower (1) four rows of the lane's eight:
// lane (lq = lane & 15, kq = lane >> 4) supplies row 32 s + 8 kq + 4 up + (lq >> 2), keys tr_key .. + 3
constexpr int tr_row(int lane, int s, int up) { return 32 * s + 8 * (lane >> 4) + 4 * up + ((lane & 15) >> 2); }
constexpr int tr_key(int lane, int h) { return 8 * (lane & 3) + 4 * (h ^ (lane & 1)); }
constexpr int tr_off(int d, int lane, int s, int h, int up, int plane) { return element(d, tr_row(lane, s, up), tr_key(lane, h), plane); }
// the keys that end in the lane's accumulator h after the matrix instruction (C: reg r of lane = row 4 kq + r): 8 kq + 4 (h ^ (kq & 1)) + r
constexpr int acc_key(int lane, int h, int r) { return 8 * (lane >> 4) + 4 * (h ^ ((lane >> 4) & 1)) + r; }

// row read of channel group c: lane (lq, kq) takes row 16 c + lq, keys 8 kq .. 8 kq + 7
constexpr int rd_row(int lane, int c) { return 16 * c + (lane & 15); }
constexpr int rd_off(int d, int lane, int c, int plane) { return element(d, rd_row(lane, c), 8 * (lane >> 4), plane); }

}  // namespace csn_tile_image
