// The uniform grid over the scene cloud: the header the build writes on the device, the layout of the caller's workspace
// (mh_scene_grid_bytes) and the cell of a point.  Internal to the library (not part of the C ABI); included by
// mh_scene.hip, which builds the grid and searches it for the contact term, and by mh_contact.hip.  The build's shared parts
// (workspace layout, box reduction, scan) are those of mh_cells_p.h.
#pragma once
#include "mh_cells_p.h"
#include "mh_common.h"

#define GRID_MAX_CELLS (1 << 20)

struct GridHdr {        // device-resident header (written by k_grid_setup)
  float mn[3];
  float cell;
  int dim[3];
  int ncells;
  int npts;          // points in the cloud (<= the capacity the workspace was sized for)
};

__device__ __forceinline__ int grid_cell(const GridHdr* h, float x, float y, float z) {
  const int cx = min(max((int)((x - h->mn[0]) / h->cell), 0), h->dim[0] - 1);
  const int cy = min(max((int)((y - h->mn[1]) / h->cell), 0), h->dim[1] - 1);
  const int cz = min(max((int)((z - h->mn[2]) / h->cell), 0), h->dim[2] - 1);
  return (cz * h->dim[1] + cy) * h->dim[0] + cx;
}

struct GridWs {
  GridHdr* hdr;
  int* start;     // [GRID_MAX_CELLS + 1]
  int* cursor;    // [GRID_MAX_CELLS]
  int* pcell;     // [M]
  float* sorted;  // [M][3]
};
static size_t grid_bytes(size_t M) { return cells_bytes(1, sizeof(GridHdr), GRID_MAX_CELLS, M * 4, M * 12); }
static GridWs grid_carve(void* ws, int M) {     // the layout of mh_cells_p.h for one body
  const CellsWs c = cells_carve(ws, 1, sizeof(GridHdr), GRID_MAX_CELLS, (size_t)M * 4);
  return {(GridHdr*)c.hdr, c.start, c.cursor, (int*)c.a, (float*)c.b};
}
