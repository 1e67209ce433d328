// ivf_filter_tile.hpp — the tile of the IVF list filter's score kernel (kernels.hpp describes what the kernel does with it), shared by
// the kernels' argument blocks and the host plan (ivf_filter_plan.hpp).  A plain struct: no HIP header, no library header but <cstdint>.
#pragma once
#include <cstdint>

namespace fsgpu {

// Up to kIvfFilterTileQueries consecutive slots of one list.
struct IvfFilterTile {
    uint64_t ordered_row0;   // the list's first row in the ordered copy
    uint64_t list_pos0;      // ... and in list_rows
    uint64_t scratch0;       // of the tile's first slot, in entries, from the start of the range the tile runs in
    uint32_t len, slot0, nmem, item0;
};

}  // namespace fsgpu
