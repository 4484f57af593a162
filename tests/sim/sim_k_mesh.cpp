// TEST INFRASTRUCTURE: mesh extraction (mesh_kernels.h) on the CPU executor.  The launch sequences repeat vmap_amd/csrc/k_mesh.hip; the
// workspace layout is the product's own (vl::mesh_layout, launch_geometry.h).
#include <cstring>

#include "launch_geometry.h"
#include "mesh_kernels.h"
#include "sim_runtime.h"

namespace {
vm::MeshArgs mesh_args(const float* volume, int nx, int ny, int nz, float level, void* workspace) {
    const vl::MeshLayout l = vl::mesh_layout(nx, ny, nz);
    vm::MeshArgs a;
    std::memset(&a, 0, sizeof(a));
    a.vol = volume; a.nx = nx; a.ny = ny; a.nz = nz; a.n = (int)l.n; a.nblk = l.nblk; a.level = level;
    char* ws = static_cast<char*>(workspace);
    a.blk = reinterpret_cast<long long*>(ws);
    a.firstv = reinterpret_cast<int*>(ws + l.off_firstv);
    a.emask = reinterpret_cast<unsigned char*>(ws + l.off_emask);
    return a;
}
}  // namespace

// out: n, nblk, off_firstv, off_emask, bytes
extern "C" void vmsim_mesh_layout(int nx, int ny, int nz, long long* out) {
    const vl::MeshLayout l = vl::mesh_layout(nx, ny, nz);
    out[0] = l.n; out[1] = l.nblk; out[2] = (long long)l.off_firstv; out[3] = (long long)l.off_emask; out[4] = (long long)l.bytes;
}

extern "C" int vmsim_mesh_grid_points(int nx, int ny, int nz, const float* affine, float* points) {
    vm::MeshArgs a = mesh_args(nullptr, nx, ny, nz, 0.0f, nullptr);
    std::memcpy(a.A, affine, sizeof(a.A));
    sim::launch(a.nblk, vm::kMeshWG, 0, [&] { vm::mesh_grid_points(a, points); });
    return 0;
}

extern "C" int vmsim_mesh_count(const float* volume, int nx, int ny, int nz, float level, long long* counts, void* workspace) {
    vm::MeshArgs a = mesh_args(volume, nx, ny, nz, level, workspace);
    a.counts = counts;
    sim::launch(a.nblk, vm::kMeshWG, 0, [&] { vm::mesh_count(a); });
    sim::launch(1, vm::kScanWG, 0, [&] { vm::mesh_scan(a); });
    return 0;
}

extern "C" int vmsim_mesh_emit(const float* volume, int nx, int ny, int nz, float level, const float* affine, const float* ninv,
                               float* vertices, float* normals, int* faces, long long n_vertices, long long n_faces, void* workspace) {
    vm::MeshArgs a = mesh_args(volume, nx, ny, nz, level, workspace);
    a.verts = vertices; a.normals = normals; a.faces = faces; a.n_vertices = n_vertices; a.n_faces = n_faces;
    if (affine) {
        std::memcpy(a.A, affine, sizeof(a.A));
        std::memcpy(a.Ninv, ninv, sizeof(a.Ninv));
        a.has_affine = 1;
    }
    sim::launch(a.nblk, vm::kMeshWG, 0, [&] { vm::mesh_emit_vertices(a); });
    if (n_faces == 0) return 0;
    sim::launch(a.nblk, vm::kMeshWG, 0, [&] { vm::mesh_emit_faces(a); });
    return 0;
}
