// Wire packing: ASCII text travels host -> device as 7 bits per byte.
//
// A strip of n bytes is cut into blocks of kWireBlock bytes (the last may be
// short).  A block whose bytes are all < 0x80 is written as 7 bytes per group
// of 8 (byte i of a group in bits 7i..7i+6 of a little-endian 56-bit value; a
// trailing group of fewer than 8 bytes is padded with zero bytes in the packed
// form only); any other block is written unchanged.  table[b] is the block's
// offset in the packed strip, with kWireRawBit set when it went unchanged.
// Every full block is 4096 or 3584 bytes, so block offsets are multiples of 16.
// The device side (wirepack.hip) restores the bytes in HBM before K1 reads them.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tsg {

constexpr uint32_t kWireBlock = 4096;
constexpr uint32_t kWireBlockPacked = kWireBlock / 8 * 7;
constexpr uint32_t kWireRawBit = 1u << 31;
constexpr uint64_t kWireMaxStrip = 1ull << 30;   // table offsets keep bit 31 for the mode
constexpr size_t kWireSlack = 64;                // pack may write, unpack may read, this far past the packed bytes

enum WirePath { kWireAuto = 0, kWireScalar = 1, kWireAvx2 = 2 };

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

}  // namespace tsg
