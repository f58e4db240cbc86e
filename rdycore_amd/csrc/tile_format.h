// The format of the tables the host writes at create and the kernels read: the neighbour encoding, the capacities every
// tile is cut to, the packed edge records and slot references, the tile descriptor and the LDS sizes that follow from the
// capacities.  Plain C++17, no HIP include: the host-side layout pass (host_layout.h) is built from this header alone, and
// the kernel headers take the same constants from here (swe_device.h includes it).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RDY_HOST_DEVICE __host__ __device__
#else
#define RDY_HOST_DEVICE
#endif

namespace rdyhip {

constexpr int32_t NBR_EMPTY = INT32_MIN;    // unused slot (triangle in a 4-slot layout)
constexpr int32_t NBR_GHOST = 1 << 30;      // neighbour is a ghost (non-owned) cell
constexpr int32_t NBR_MASK  = (1 << 30) - 1;

constexpr int BLOCK = 256;  // threads per workgroup of the cell-centric kernel
constexpr int TILE = 256;   // threads per workgroup of the tiled kernels = the largest number of cells in a tile (a multiple of 64)
// Capacities every tile is cut to at create (layout_build_tiles): edge records = two register-resident rounds of the edge
// phase; halo cells (cells outside the tile that share an edge with it) per slots-per-cell flavour.  The LDS planes have
// these compile-time lengths, so every plane offset is an instruction immediate.
constexpr int TILE_MAX_REC = 2 * TILE;
constexpr int TILE_MAX_HALO_TRI = 104, TILE_MAX_HALO_QUAD = 112;

constexpr uint16_t SLOT_EMPTY = 0xFFFF;

// packed end points of a tile edge: LDS slot of the left cell | slot of the
// right cell << 11 | EDGE_BOUNDARY.  Slots 0..255 are the tile's own cells,
// 256.. the tile's halo cells (cells outside the tile that share an edge with
// it).  For a boundary edge the right field is the index into the tile's
// boundary-edge list.
constexpr uint32_t EDGE_SLOT_MASK = 0x7FF;
constexpr int      EDGE_R_SHIFT   = 11;
constexpr uint32_t EDGE_BOUNDARY  = 1u << 22;
// The unit normal (cn, sn) is stored as ONE double: the component of smaller
// magnitude; the other is +-sqrt(1 - cs^2) (well conditioned: cs^2 <= 1/2).
constexpr uint32_t EDGE_CS_IS_CN     = 1u << 23;  // the stored component is cn (else sn)
constexpr uint32_t EDGE_OTHER_NEG    = 1u << 24;  // the reconstructed component is negative
// second order: the edge belongs to another rank (edges.is_owned = false): ApplyInteriorFlux2R evaluates its Courant number
// there (swe_petsc.c:172-190); here its flux still feeds the owned cell, its wave speed is kept out of the diagnostic
constexpr uint32_t EDGE_NOT_OWNED    = 1u << 25;
// Normal table (normal_table.h): where the edges of a mesh have at most NORMAL_TABLE_MAX distinct (stored component, CS_IS_CN,
// OTHER_NEG) triples -- a raster-derived mesh has six or eight -- bits 26-31 of a record's word hold the index of its triple
// in a table of the operator (ColdArgs::nt_*), and the first-order / HR table kernels (swe_rhs_ntab_kernel) do not read e_cs.
// Every other reader masks the fields it uses, so the words serve both families.
constexpr int      NORMAL_TABLE_MAX   = 64;
constexpr int      EDGE_NT_SHIFT      = 26;
constexpr uint32_t EDGE_NT_FLAGS      = EDGE_CS_IS_CN | EDGE_OTHER_NEG;  // what a table entry keeps of a word
// slot references of a triangle mesh (S == 3): 3 x 10 bits in one uint32, 0x3FF = unused
constexpr uint32_t REF3_EMPTY = 0x3FF;

struct TileDesc {  // 16 B, one per tile (+1 sentinel): everything about a tile in ONE scalar load of four registers
  int32_t  e_off;  // first edge record
  int32_t  h_off;  // first halo-cell entry
  int32_t  c_off;  // first owned cell (the tile's cells are c_off .. c_off + nc() - 1; a multiple of 16 wherever the numbering allows)
  uint32_t cnt;    // edge records (bits 0-10) | halo cells (bits 11-21) | cells - 1 (bits 22-29) | bit 30: a tile cell is sent to
                   // another rank (set while a halo with the fused pack is attached) | bit 31: a tile cell has a ghost neighbour
  RDY_HOST_DEVICE int  ne() const { return (int)(cnt & 0x7FFu); }
  RDY_HOST_DEVICE int  nh() const { return (int)((cnt >> 11) & 0x7FFu); }
  RDY_HOST_DEVICE int  nc() const { return (int)((cnt >> 22) & 0xFFu) + 1; }
  RDY_HOST_DEVICE bool halo() const { return (cnt >> 31) != 0; }
  RDY_HOST_DEVICE bool send() const { return ((cnt >> 30) & 1u) != 0; }
};
constexpr uint32_t TILE_HALO_FLAG = 1u << 31;
constexpr uint32_t TILE_SEND_FLAG = 1u << 30;

// LDS of the first-order / HR tiled kernels: planes per cell slot (own + halo cells), per own cell and per edge record
constexpr int TILED_NS_TRI = TILE + TILE_MAX_HALO_TRI, TILED_NS_QUAD = TILE + TILE_MAX_HALO_QUAD, TILED_NE = TILE_MAX_REC + 8;
constexpr size_t tiled_lds_bytes(int S, bool hr) {
  return sizeof(double) * ((hr ? 6 : 5) * (size_t)(S == 3 ? TILED_NS_TRI : TILED_NS_QUAD) + 2 * (size_t)TILE + (hr ? 6 : 4) * (size_t)TILED_NE);
}
// ... of the table kernels: the same planes, then the (cn, sn) pairs of the normal table, 16 B each (the planes end on a
// multiple of 16 B in all four families)
constexpr size_t tiled_ntab_lds_bytes(int S, bool hr) { return tiled_lds_bytes(S, hr) + 2 * sizeof(double) * (size_t)NORMAL_TABLE_MAX; }
static_assert(tiled_lds_bytes(3, false) % 16 == 0 && tiled_lds_bytes(3, true) % 16 == 0 && tiled_lds_bytes(4, false) % 16 == 0 &&
                  tiled_lds_bytes(4, true) % 16 == 0 && tiled_ntab_lds_bytes(4, true) <= 64 * 1024,
              "the planes ahead of the normal table are a multiple of 16 B (the array itself is declared aligned(16)), and the table fits a workgroup's 64 KB");

// second order (muscl_kernels.h): MusclArgs::bn_idx entries that are no LDS slot
constexpr uint16_t BN_NONE = 0xFFFF, BN_GLOBAL = 0xFFFE;
// triangles: 256 own + <= 104 first-ring cells, <= 264 ring cells in all, <= 512 edge records (two register rounds)
// (every ring cell is staged by one thread: at most TILE of them)
constexpr int MUSCL_MAX_RING1_TRI = TILE_MAX_HALO_TRI, MUSCL_MAX_RING_TRI = TILE;
// quads / mixed meshes: <= 112 first-ring cells, <= 168 ring cells in all
constexpr int MUSCL_MAX_RING1_QUAD = TILE_MAX_HALO_QUAD, MUSCL_MAX_RING_QUAD = 168;
// LDS of the second-order kernel (MusclSoATri / MusclSoAQuad of muscl_kernels.h, which asserts the equality): six gradient
// planes over own + first-ring cells, five state planes over own + both rings (the triangles' keep 8 slots of slack), one
// 4-byte plane over the edge records
constexpr size_t muscl_lds_bytes(int S) {
  return sizeof(double) * (6 * (size_t)(TILE + (S == 3 ? MUSCL_MAX_RING1_TRI : MUSCL_MAX_RING1_QUAD)) +
                           5 * (size_t)(TILE + (S == 3 ? MUSCL_MAX_RING_TRI + 8 : MUSCL_MAX_RING_QUAD))) +
         sizeof(uint32_t) * (size_t)(TILE_MAX_REC + 8);
}

}  // namespace rdyhip
