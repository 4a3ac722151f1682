// Stand-alone host driver around objcavit_amd/csrc/union_find.hpp (tests/test_obstacles_host.py builds it with the system C++ compiler
// under -fsanitize=address,undefined and runs it as a process of its own).  It labels a grid the way csrc/obstacles.hip does -- per tile
// on tile-local indices, the tile roots written out as linear indices of the grid, then the pairs across tile edges on those -- with the
// header's own find / union, one caller at a time.
//   stdin:  GX GY link tile, then GY * GX cells (0 / 1, row-major)
//   stdout: GY * GX roots (the smallest iy * GX + ix of the cell's component, -1 for an empty cell)
#include <cstdio>
#include <vector>

#include "union_find.hpp"

int main() {
  int GX, GY, link, tile;
  if (std::scanf("%d %d %d %d", &GX, &GY, &link, &tile) != 4 || GX < 1 || GY < 1 || link < 1 || tile < 1) return 2;
  std::vector<int> occ((size_t)GX * GY), parent((size_t)GX * GY, -1);
  for (int& v : occ)
    if (std::scanf("%d", &v) != 1) return 2;
  // the tile pass
  std::vector<int> local((size_t)tile * tile);
  for (int gy0 = 0; gy0 < GY; gy0 += tile)
    for (int gx0 = 0; gx0 < GX; gx0 += tile) {
      auto at = [&](int ly, int lx) { return gy0 + ly < GY && gx0 + lx < GX && occ[(size_t)(gy0 + ly) * GX + gx0 + lx] != 0; };
      for (int l = 0; l < tile * tile; ++l) local[l] = l;
      for (int l = 0; l < tile * tile; ++l) {
        const int ly = l / tile, lx = l % tile;
        if (!at(ly, lx)) continue;
        for (int dy = 0; dy <= link && ly + dy < tile; ++dy)
          for (int dx = dy == 0 ? 1 : -link; dx <= link; ++dx) {
            const int nx = lx + dx;
            if (nx < 0 || nx >= tile) continue;
            if (at(ly + dy, nx)) uf_union(local.data(), l, (ly + dy) * tile + nx);
          }
      }
      for (int l = 0; l < tile * tile; ++l) {
        const int ly = l / tile, lx = l % tile;
        if (!at(ly, lx)) continue;
        const int r = uf_find(local.data(), l);
        parent[(size_t)(gy0 + ly) * GX + gx0 + lx] = (gy0 + r / tile) * GX + gx0 + r % tile;
      }
    }
  // the seam pass
  for (int gy = 0; gy < GY; ++gy)
    for (int gx = 0; gx < GX; ++gx) {
      if (!occ[(size_t)gy * GX + gx]) continue;
      for (int dy = 0; dy <= link && gy + dy < GY; ++dy)
        for (int dx = dy == 0 ? 1 : -link; dx <= link; ++dx) {
          const int nx = gx + dx, ny = gy + dy;
          if (nx < 0 || nx >= GX) continue;
          if (nx / tile == gx / tile && ny / tile == gy / tile) continue;
          if (occ[(size_t)ny * GX + nx]) uf_union(parent.data(), gy * GX + gx, ny * GX + nx);
        }
    }
  for (int c = 0; c < GX * GY; ++c) std::printf("%d\n", occ[c] ? uf_find(parent.data(), c) : -1);
  return 0;
}
