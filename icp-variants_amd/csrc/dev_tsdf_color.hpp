// dev_tsdf_color.hpp -- the byte rule of the coloured model (icp_tsdf_raycast_color, icp_tsdf_mesh_color): a running-average channel to
// its byte and three of them to the packed word the clouds hold.  Contract: include/icp_hip.h, DESIGN.md section 6p.
// Part of icp_device.hpp (included from there, inside namespace icpdev, before dev_tsdf.hpp).
__device__ __forceinline__ uint32_t tsdf_color_byte(float c) { return (uint32_t)(uint8_t)(int)floorf(fminf(fmaxf(c, 0.f), 255.f) + 0.5f); }
// R | G << 8 | B << 16 | 255 << 24: never 0, which stands for "no colour"
__device__ __forceinline__ uint32_t tsdf_color_pack(float r, float g, float b) {
    return tsdf_color_byte(r) | (tsdf_color_byte(g) << 8) | (tsdf_color_byte(b) << 16) | 0xFF000000u;
}
