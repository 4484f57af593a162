// k_mesh.hip - mesh extraction (mesh_kernels.h): the grid Trainer.meshing queries and marching cubes as count -> scan -> emit.
// gfx950 only.
#include <cstring>

#include "../../include/vmapstep.h"
#include "launch.h"
#include "mesh_kernels.h"

namespace vl {

static vm::MeshArgs mesh_args(const float* volume, int nx, int ny, int nz, float level, void* workspace) {
    const MeshLayout l = mesh_layout(nx, ny, nz);
    vm::MeshArgs a;
    std::memset(&a, 0, sizeof(a));
    a.vol = volume; a.nx = nx; a.ny = ny; a.nz = nz; a.n = (int)l.n; a.nblk = l.nblk; a.level = level;
    char* ws = static_cast<char*>(workspace);
    a.blk = reinterpret_cast<long long*>(ws);
    a.firstv = reinterpret_cast<int*>(ws + l.off_firstv);
    a.emask = reinterpret_cast<unsigned char*>(ws + l.off_emask);
    return a;
}

int mesh_grid_points(int nx, int ny, int nz, const float affine[12], float* points, hipStream_t st) {
    vm::MeshArgs a = mesh_args(nullptr, nx, ny, nz, 0.0f, nullptr);
    std::memcpy(a.A, affine, sizeof(a.A));
    hipLaunchKernelGGL(vm::mesh_grid_points, dim3(a.nblk), dim3(vm::kMeshWG), 0, st, a, points);
    return launched("mesh_grid_points");
}

int mesh_count(const float* volume, const unsigned char* valid, int nx, int ny, int nz, float level, long long* counts, void* workspace,
               hipStream_t st) {
    vm::MeshArgs a = mesh_args(volume, nx, ny, nz, level, workspace);
    a.valid = valid;
    a.counts = counts;
    hipLaunchKernelGGL(vm::mesh_count, dim3(a.nblk), dim3(vm::kMeshWG), 0, st, a);
    if (int rc = launched("mesh_count")) return rc;
    hipLaunchKernelGGL(vm::mesh_scan, dim3(1), dim3(vm::kScanWG), 0, st, a);
    return launched("mesh_scan");
}

int mesh_emit(const float* volume, const unsigned char* valid, int nx, int ny, int nz, float level, const float* affine, const float* ninv,
              float* vertices, float* normals, int* faces, int* edge_ids, long long n_vertices, long long n_faces, void* workspace,
              hipStream_t st) {
    vm::MeshArgs a = mesh_args(volume, nx, ny, nz, level, workspace);
    a.valid = valid; a.edge_ids = edge_ids;
    a.verts = vertices; a.normals = normals; a.faces = faces; a.n_vertices = n_vertices; a.n_faces = n_faces;
    if (affine) {
        std::memcpy(a.A, affine, sizeof(a.A));
        std::memcpy(a.Ninv, ninv, sizeof(a.Ninv));
        a.has_affine = 1;
    }
    // faces read the vertex ids emit_vertices records: two launches, so no workgroup waits on another of the same launch
    hipLaunchKernelGGL(vm::mesh_emit_vertices, dim3(a.nblk), dim3(vm::kMeshWG), 0, st, a);
    if (int rc = launched("mesh_emit_vertices")) return rc;
    if (n_faces == 0) return VMAPSTEP_OK;
    hipLaunchKernelGGL(vm::mesh_emit_faces, dim3(a.nblk), dim3(vm::kMeshWG), 0, st, a);
    return launched("mesh_emit_faces");
}

}  // namespace vl
