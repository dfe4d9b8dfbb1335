// What the mesh rasteriser (render.hip) leaves behind for the kernels that run after it on the same chunk (shade.hip): the tile
// shape and the layout of the per-window scratch that ev2h_render_scratch_bytes sizes.
#pragma once

constexpr int RND_THREADS = 256;
constexpr int RND_TILE_W = 16, RND_TILE_H = 16;         // one pixel per thread; measured: 16x16 0.605 ms, 32x8 0.724, 64x4 0.73 per 256 windows
constexpr int RND_MAX_VERTS = 2048;                     // LDS image of the projected vertices: 16 B each
constexpr int RND_HEADER_FLOATS = 8;                    // per-window scratch: [x0, y0, x1, y1 of the screen bounding box, 4 unused]
constexpr int RND_RECORD_FLOATS = 8;                    // then per vertex (u, v, 1/z_mm or 0 = behind znear, 0, nx, ny, nz, 0)
