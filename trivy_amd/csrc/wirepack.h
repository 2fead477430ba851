// Wire packing: text travels host -> device in fewer bits than it has.  Two
// codecs share the strip / block / table structure; the engine picks one per
// scan (TSG_WIRE_PACK).
//
// ---- the 7-bit codec (wire_pack / wire_unpack)
//
// A strip of n bytes is cut into blocks of kWireBlock bytes (the last may be
// short).  A block whose bytes are all < 0x80 is written as 7 bytes per group
// of 8 (byte i of a group in bits 7i..7i+6 of a little-endian 56-bit value; a
// trailing group of fewer than 8 bytes is padded with zero bytes in the packed
// form only); any other block is written unchanged.  table[b] is the block's
// offset in the packed strip, with kWireRawBit set when it went unchanged.
// Every full block is 4096 or 3584 bytes, so block offsets are multiples of 16.
// The device side (wirepack.hip) restores the bytes in HBM before K1 reads them.
//
// ---- the 6-bit codec with escapes, "v2" (wire_pack2 / wire_unpack2)
//
// The same strip, blocks and table.  The strip is also cut into regions of
// kWire2Region bytes (16 blocks; the last may be short), each with an alphabet
// of 63 byte values < 0x80:
//
//   * the region's bytes at offsets 0, kWire2Sample, 2 kWire2Sample, ... from
//     the region's start are counted (bytes >= 0x80 are skipped);
//   * the 128 values are ordered by count, larger first, equal counts by value,
//     lower first (values that were never seen follow in value order);
//   * alphabet[c] is the c-th of them, c = 0..62; alphabet[63] is zero.
//
// The alphabets (64 bytes per region, region order) form the strip's second
// head: wire2_alpha_bytes(n) bytes, which travel between the table and the
// packed bytes.
//
// A block of len bytes is written in the smallest of its modes (three, or four
// where split blocks are allowed; the tie order follows the list):
//
//   * raw (kWireRawBit): len bytes unchanged;
//   * 7-bit (no mode bit): as above, (len + 7) / 8 * 7 bytes; only for a block
//     whose bytes are all < 0x80;
//   * 6-bit (kWire6Bit): byte k of the block becomes a 6-bit code in bits
//     6k .. 6k+5 of a little-endian bit string of (len + 3) / 4 * 3 bytes (codes
//     past len are zero), padded with zero bytes to a multiple of 16.  Code c <
//     63 stands for alphabet[c] of the block's region; code 63 for the next of
//     the block's escaped bytes, which follow the codes in block order, padded
//     with zero bytes to a multiple of 16.  A byte escapes exactly when it is
//     not among the region's 63 alphabet values.  With e escaped bytes the size
//     is pad16((len + 3) / 4 * 3) + pad16(e): a full block goes 6-bit instead of
//     7-bit up to e = 496 and instead of raw up to e = 1008.
//
//   * split (kWireRawBit and kWire6Bit both set; only where the packer is
//     allowed to, see wire_pack2): the codes are those of the 6-bit mode, that
//     is positions in the region's alphabet.  A byte is "hot" when its code is
//     below 16, "warm" when it is 16..46; every other byte (code 47..62, or
//     not in the alphabet) escapes.  With h hot bytes and e escaping ones the
//     block is four streams laid back to back at byte granularity, every pad
//     bit zero, the total padded with zero bytes to a multiple of 16:
//       - the mask, (len + 7) / 8 bytes: bit k % 8 of byte k / 8 is set when
//         byte k of the block is hot;
//       - the hot codes in block order, 4 bits each, the j-th in bits 4j ..
//         4j+3 of a little-endian bit string of (h + 1) / 2 bytes;
//       - one 5-bit value for every other byte in block order, the j-th in
//         bits 5j .. 5j+4 of a little-endian bit string of
//         (5 (len - h) + 7) / 8 bytes: code - 16 for a warm byte, 31 for one
//         that escapes;
//       - the e escaping bytes in block order.
//     The size is wire2_split_bytes(len, h, e) =
//       pad16((len + 7) / 8 + (h + 1) / 2 + (5 (len - h) + 7) / 8 + e),
//     for a full block pad16(3072 - h / 8 + e) where h is a multiple of 8.
//
// Of equal sizes raw is preferred to 7-bit, 7-bit to 6-bit and 6-bit to split.
//
// table[b] = offset | mode bits.  Every block has a size that is a multiple of
// 16 except a strip's last (raw or 7-bit), so offsets are multiples of 16, and
// they stay below 2^30.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tsg {

constexpr uint32_t kWireBlock = 4096;
constexpr uint32_t kWireBlockPacked = kWireBlock / 8 * 7;
constexpr uint32_t kWireRawBit = 1u << 31;
constexpr uint64_t kWireMaxStrip = 1ull << 30;   // table offsets keep bits 30 and 31 for the mode
constexpr size_t kWireSlack = 64;                // pack may write, unpack may read, this far past the packed bytes

enum WirePath { kWireAuto = 0, kWireScalar = 1, kWireAvx2 = 2, kWireVbmi = 3 };

inline size_t wire_blocks(size_t n) { return (n + kWireBlock - 1) / kWireBlock; }
inline size_t wire_packed_len(size_t block_bytes) { return (block_bytes + 7) / 8 * 7; }
// bytes a destination must have for a strip of n bytes
inline size_t wire_bound(size_t n) { return n + 8 + kWireSlack; }
// the table's share of a strip's staging / landing buffer (the packed bytes follow it)
inline size_t wire_table_bytes(size_t n) { return (wire_blocks(n) * sizeof(uint32_t) + 255) & ~size_t(255); }

bool wire_have_avx2();
// Packs src[0, n) into dst (wire_bound(n) bytes) and table (wire_blocks(n)
// entries); returns the packed length.  src needs no alignment.  Both paths
// give the same bytes; kWireAvx2 on a CPU without AVX2 runs the scalar path.
size_t wire_pack(const uint8_t* src, size_t n, uint8_t* dst, uint32_t* table, int path);
// The reference unpack: dst[0, n) from a packed strip.
void wire_unpack(const uint8_t* packed, const uint32_t* table, size_t n, uint8_t* dst);

// Test hook (wirepack.hip): uploads a packed strip (table + bytes) to device
// 0, runs the unpack kernel and reads the n restored bytes back into out.
bool wire_unpack_device_probe(const uint8_t* packed, size_t packed_len, const uint32_t* table, size_t n, uint8_t* out,
                              const char** err);

// ---- v2

constexpr uint32_t kWire6Bit = 1u << 30;
constexpr uint32_t kWire2Region = 65536;         // bytes per alphabet
constexpr uint32_t kWire2Sample = 64;            // every 64th byte of a region is counted
constexpr uint32_t kWire2Alpha = 64;             // bytes per stored alphabet (63 values and a zero)
constexpr uint32_t kWire2Escape = 63;

struct Wire2Stats {
  uint64_t blocks6 = 0, blocks7 = 0, blocks_raw = 0;
  uint64_t escaped = 0;                          // escaped bytes of the 6-bit and split blocks
  uint64_t blocks_split = 0;
};

inline size_t wire2_regions(size_t n) { return (n + kWire2Region - 1) / kWire2Region; }
inline size_t wire2_alpha_bytes(size_t n) { return (wire2_regions(n) * kWire2Alpha + 255) & ~size_t(255); }
inline size_t wire2_code_bytes(size_t block_bytes) { return ((block_bytes + 3) / 4 * 3 + 15) & ~size_t(15); }
inline size_t wire2_bound(size_t n) { return n + 16 + kWireSlack; }
constexpr uint32_t kWire2Hot = 16;               // split mode: codes below it go in 4 bits
constexpr uint32_t kWire2Warm = 47;              // codes kWire2Hot .. kWire2Warm - 1 go in 5 bits; the rest escape
constexpr uint32_t kWire2Escape5 = 31;
// a split block of len bytes, h of them hot and e escaping
inline size_t wire2_split_bytes(size_t len, size_t h, size_t e) {
  return ((len + 7) / 8 + (h + 1) / 2 + (5 * (len - h) + 7) / 8 + e + 15) & ~size_t(15);
}

bool wire_have_vbmi();
// AVX-512 VBMI2 (byte compress) besides what wire_have_vbmi() asks for: the
// kWireVbmi path then packs split blocks, and the escaped bytes of 6-bit ones,
// with it; without it split blocks are packed by the AVX2 path.
bool wire_have_vbmi2();
// The path wire_pack2 runs for a requested one: the request itself where the
// CPU has it, else the best below it (kWireAuto: the CPU's best).
int wire2_path(int path);
// Packs src[0, n) into dst (wire2_bound(n) bytes), table (wire_blocks(n)
// entries) and alpha (wire2_alpha_bytes(n) bytes, written whole); returns the
// packed length.  Every path gives the same bytes.  Split blocks are written
// only with `split` set; without it the bytes are those of the three modes.
size_t wire_pack2(const uint8_t* src, size_t n, uint8_t* dst, uint32_t* table, uint8_t* alpha, int path,
                  Wire2Stats* stats, bool split = false);
// The reference unpack; reads nothing past the packed bytes.
void wire_unpack2(const uint8_t* packed, const uint32_t* table, const uint8_t* alpha, size_t n, uint8_t* dst);
// As wire_unpack_device_probe, with the v2 kernel.
bool wire_unpack2_device_probe(const uint8_t* packed, size_t packed_len, const uint32_t* table, const uint8_t* alpha,
                               size_t n, uint8_t* out, const char** err);

}  // namespace tsg
