// mesh_kernels.h - marching cubes over a dense occupancy grid: what the reference's Trainer.meshing (trainer.py:35-75) hands
// to skimage.measure.marching_cubes on the host (vis.py:6-19), on the device.
//
// Four launches per mesh, none of which hands data to another workgroup of the same launch (no atomics decide where output goes,
// so the output is bit-identical from call to call and independent of dispatch order):
//   mesh_count          per grid point: which of its three +axis edges cross the level (it owns them) and, for the cell whose lowest
//                       corner it is, the triangle count of the cell's cube index; per-workgroup totals to the workspace
//   mesh_scan           one workgroup: exclusive scan of the workgroup totals (both columns in one pass), grand totals (vertices,
//                       faces) to a device int64[2]
//   mesh_emit_vertices  workgroup scan + workgroup offset -> the vertex id of every crossing edge; position and normal written
//   mesh_emit_faces     workgroup scan + workgroup offset -> face ids; the classic table's triangles as the owners' vertex ids
// Output order: vertices by owning point (i * ny + j) * nz + k, then axis 0, 1, 2; faces by cell (= its lowest corner's index),
// then table order.  Every kernel handles one grid point per thread, kMeshWG points per workgroup.  The workgroup scans and the scan
// of the totals are scan_ops.h's (wave shuffles, one LDS word per wave).
#pragma once
#include <hip/hip_runtime.h>

#include "launch_geometry.h"
#include "scan_ops.h"

namespace vm {

// The classic (Lorensen) triangle table: for each cube index (bit c set iff corner c lies strictly above the level), up to five
// triangles as edge ids, -1 terminated.  Corners and edges are numbered as in Lorensen & Cline / Bourke's table with x along the
// volume's LAST axis (k), y along j, z along i:
//   corner c: (di, dj, dk) = 0 (0,0,0)  1 (0,0,1)  2 (0,1,1)  3 (0,1,0)  4 (1,0,0)  5 (1,0,1)  6 (1,1,1)  7 (1,1,0)
//   edge e:   0 c0-c1  1 c1-c2  2 c2-c3  3 c3-c0  4 c4-c5  5 c5-c6  6 c6-c7  7 c7-c4  8 c0-c4  9 c1-c5  10 c2-c6  11 c3-c7
// The rows are scikit-image's CASESCLASSIC (skimage/measure/_marching_cubes_lewiner_luts.py, the table its method='lorensen' uses),
// distributed under the following licence:
//
//   Copyright (C) 2019, the scikit-image team. All rights reserved.
//   Redistribution and use in source and binary forms, with or without modification, are permitted provided that the following
//   conditions are met:
//    1. Redistributions of source code must retain the above copyright notice, this list of conditions and the following disclaimer.
//    2. Redistributions in binary form must reproduce the above copyright notice, this list of conditions and the following
//       disclaimer in the documentation and/or other materials provided with the distribution.
//    3. Neither the name of skimage nor the names of its contributors may be used to endorse or promote products derived from this
//       software without specific prior written permission.
//   THIS SOFTWARE IS PROVIDED BY THE AUTHOR ``AS IS'' AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT NOT LIMITED TO, THE
//   IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR A PARTICULAR PURPOSE ARE DISCLAIMED. IN NO EVENT SHALL THE AUTHOR BE LIABLE
//   FOR ANY DIRECT, INDIRECT, INCIDENTAL, SPECIAL, EXEMPLARY, OR CONSEQUENTIAL DAMAGES (INCLUDING, BUT NOT LIMITED TO, PROCUREMENT OF
//   SUBSTITUTE GOODS OR SERVICES; LOSS OF USE, DATA, OR PROFITS; OR BUSINESS INTERRUPTION) HOWEVER CAUSED AND ON ANY THEORY OF
//   LIABILITY, WHETHER IN CONTRACT, STRICT LIABILITY, OR TORT (INCLUDING NEGLIGENCE OR OTHERWISE) ARISING IN ANY WAY OUT OF THE USE OF
//   THIS SOFTWARE, EVEN IF ADVISED OF THE POSSIBILITY OF SUCH DAMAGE.
// (tests/mesh_oracle.py reads the rows from this file; tests/test_mesh.py checks the oracle against scikit-image's own output.)
__constant__ signed char kMcTri[256][16] = {
    {-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,1,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,8,3,9,8,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,1,2,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,2,10,0,2,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,8,3,2,10,8,10,9,8,-1,-1,-1,-1,-1,-1,-1},
    {3,11,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,11,2,8,11,0,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,9,0,2,3,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,11,2,1,9,11,9,8,11,-1,-1,-1,-1,-1,-1,-1},
    {3,10,1,11,10,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,10,1,0,8,10,8,11,10,-1,-1,-1,-1,-1,-1,-1},
    {3,9,0,3,11,9,11,10,9,-1,-1,-1,-1,-1,-1,-1},
    {9,8,10,10,8,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,7,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,3,0,7,3,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,1,9,8,4,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,1,9,4,7,1,7,3,1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,8,4,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,4,7,3,0,4,1,2,10,-1,-1,-1,-1,-1,-1,-1},
    {9,2,10,9,0,2,8,4,7,-1,-1,-1,-1,-1,-1,-1},
    {2,10,9,2,9,7,2,7,3,7,9,4,-1,-1,-1,-1},
    {8,4,7,3,11,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {11,4,7,11,2,4,2,0,4,-1,-1,-1,-1,-1,-1,-1},
    {9,0,1,8,4,7,2,3,11,-1,-1,-1,-1,-1,-1,-1},
    {4,7,11,9,4,11,9,11,2,9,2,1,-1,-1,-1,-1},
    {3,10,1,3,11,10,7,8,4,-1,-1,-1,-1,-1,-1,-1},
    {1,11,10,1,4,11,1,0,4,7,11,4,-1,-1,-1,-1},
    {4,7,8,9,0,11,9,11,10,11,0,3,-1,-1,-1,-1},
    {4,7,11,4,11,9,9,11,10,-1,-1,-1,-1,-1,-1,-1},
    {9,5,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,5,4,0,8,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,5,4,1,5,0,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {8,5,4,8,3,5,3,1,5,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,9,5,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,0,8,1,2,10,4,9,5,-1,-1,-1,-1,-1,-1,-1},
    {5,2,10,5,4,2,4,0,2,-1,-1,-1,-1,-1,-1,-1},
    {2,10,5,3,2,5,3,5,4,3,4,8,-1,-1,-1,-1},
    {9,5,4,2,3,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,11,2,0,8,11,4,9,5,-1,-1,-1,-1,-1,-1,-1},
    {0,5,4,0,1,5,2,3,11,-1,-1,-1,-1,-1,-1,-1},
    {2,1,5,2,5,8,2,8,11,4,8,5,-1,-1,-1,-1},
    {10,3,11,10,1,3,9,5,4,-1,-1,-1,-1,-1,-1,-1},
    {4,9,5,0,8,1,8,10,1,8,11,10,-1,-1,-1,-1},
    {5,4,0,5,0,11,5,11,10,11,0,3,-1,-1,-1,-1},
    {5,4,8,5,8,10,10,8,11,-1,-1,-1,-1,-1,-1,-1},
    {9,7,8,5,7,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,3,0,9,5,3,5,7,3,-1,-1,-1,-1,-1,-1,-1},
    {0,7,8,0,1,7,1,5,7,-1,-1,-1,-1,-1,-1,-1},
    {1,5,3,3,5,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,7,8,9,5,7,10,1,2,-1,-1,-1,-1,-1,-1,-1},
    {10,1,2,9,5,0,5,3,0,5,7,3,-1,-1,-1,-1},
    {8,0,2,8,2,5,8,5,7,10,5,2,-1,-1,-1,-1},
    {2,10,5,2,5,3,3,5,7,-1,-1,-1,-1,-1,-1,-1},
    {7,9,5,7,8,9,3,11,2,-1,-1,-1,-1,-1,-1,-1},
    {9,5,7,9,7,2,9,2,0,2,7,11,-1,-1,-1,-1},
    {2,3,11,0,1,8,1,7,8,1,5,7,-1,-1,-1,-1},
    {11,2,1,11,1,7,7,1,5,-1,-1,-1,-1,-1,-1,-1},
    {9,5,8,8,5,7,10,1,3,10,3,11,-1,-1,-1,-1},
    {5,7,0,5,0,9,7,11,0,1,0,10,11,10,0,-1},
    {11,10,0,11,0,3,10,5,0,8,0,7,5,7,0,-1},
    {11,10,5,7,11,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {10,6,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,5,10,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,0,1,5,10,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,8,3,1,9,8,5,10,6,-1,-1,-1,-1,-1,-1,-1},
    {1,6,5,2,6,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,6,5,1,2,6,3,0,8,-1,-1,-1,-1,-1,-1,-1},
    {9,6,5,9,0,6,0,2,6,-1,-1,-1,-1,-1,-1,-1},
    {5,9,8,5,8,2,5,2,6,3,2,8,-1,-1,-1,-1},
    {2,3,11,10,6,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {11,0,8,11,2,0,10,6,5,-1,-1,-1,-1,-1,-1,-1},
    {0,1,9,2,3,11,5,10,6,-1,-1,-1,-1,-1,-1,-1},
    {5,10,6,1,9,2,9,11,2,9,8,11,-1,-1,-1,-1},
    {6,3,11,6,5,3,5,1,3,-1,-1,-1,-1,-1,-1,-1},
    {0,8,11,0,11,5,0,5,1,5,11,6,-1,-1,-1,-1},
    {3,11,6,0,3,6,0,6,5,0,5,9,-1,-1,-1,-1},
    {6,5,9,6,9,11,11,9,8,-1,-1,-1,-1,-1,-1,-1},
    {5,10,6,4,7,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,3,0,4,7,3,6,5,10,-1,-1,-1,-1,-1,-1,-1},
    {1,9,0,5,10,6,8,4,7,-1,-1,-1,-1,-1,-1,-1},
    {10,6,5,1,9,7,1,7,3,7,9,4,-1,-1,-1,-1},
    {6,1,2,6,5,1,4,7,8,-1,-1,-1,-1,-1,-1,-1},
    {1,2,5,5,2,6,3,0,4,3,4,7,-1,-1,-1,-1},
    {8,4,7,9,0,5,0,6,5,0,2,6,-1,-1,-1,-1},
    {7,3,9,7,9,4,3,2,9,5,9,6,2,6,9,-1},
    {3,11,2,7,8,4,10,6,5,-1,-1,-1,-1,-1,-1,-1},
    {5,10,6,4,7,2,4,2,0,2,7,11,-1,-1,-1,-1},
    {0,1,9,4,7,8,2,3,11,5,10,6,-1,-1,-1,-1},
    {9,2,1,9,11,2,9,4,11,7,11,4,5,10,6,-1},
    {8,4,7,3,11,5,3,5,1,5,11,6,-1,-1,-1,-1},
    {5,1,11,5,11,6,1,0,11,7,11,4,0,4,11,-1},
    {0,5,9,0,6,5,0,3,6,11,6,3,8,4,7,-1},
    {6,5,9,6,9,11,4,7,9,7,11,9,-1,-1,-1,-1},
    {10,4,9,6,4,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,10,6,4,9,10,0,8,3,-1,-1,-1,-1,-1,-1,-1},
    {10,0,1,10,6,0,6,4,0,-1,-1,-1,-1,-1,-1,-1},
    {8,3,1,8,1,6,8,6,4,6,1,10,-1,-1,-1,-1},
    {1,4,9,1,2,4,2,6,4,-1,-1,-1,-1,-1,-1,-1},
    {3,0,8,1,2,9,2,4,9,2,6,4,-1,-1,-1,-1},
    {0,2,4,4,2,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {8,3,2,8,2,4,4,2,6,-1,-1,-1,-1,-1,-1,-1},
    {10,4,9,10,6,4,11,2,3,-1,-1,-1,-1,-1,-1,-1},
    {0,8,2,2,8,11,4,9,10,4,10,6,-1,-1,-1,-1},
    {3,11,2,0,1,6,0,6,4,6,1,10,-1,-1,-1,-1},
    {6,4,1,6,1,10,4,8,1,2,1,11,8,11,1,-1},
    {9,6,4,9,3,6,9,1,3,11,6,3,-1,-1,-1,-1},
    {8,11,1,8,1,0,11,6,1,9,1,4,6,4,1,-1},
    {3,11,6,3,6,0,0,6,4,-1,-1,-1,-1,-1,-1,-1},
    {6,4,8,11,6,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {7,10,6,7,8,10,8,9,10,-1,-1,-1,-1,-1,-1,-1},
    {0,7,3,0,10,7,0,9,10,6,7,10,-1,-1,-1,-1},
    {10,6,7,1,10,7,1,7,8,1,8,0,-1,-1,-1,-1},
    {10,6,7,10,7,1,1,7,3,-1,-1,-1,-1,-1,-1,-1},
    {1,2,6,1,6,8,1,8,9,8,6,7,-1,-1,-1,-1},
    {2,6,9,2,9,1,6,7,9,0,9,3,7,3,9,-1},
    {7,8,0,7,0,6,6,0,2,-1,-1,-1,-1,-1,-1,-1},
    {7,3,2,6,7,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,3,11,10,6,8,10,8,9,8,6,7,-1,-1,-1,-1},
    {2,0,7,2,7,11,0,9,7,6,7,10,9,10,7,-1},
    {1,8,0,1,7,8,1,10,7,6,7,10,2,3,11,-1},
    {11,2,1,11,1,7,10,6,1,6,7,1,-1,-1,-1,-1},
    {8,9,6,8,6,7,9,1,6,11,6,3,1,3,6,-1},
    {0,9,1,11,6,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {7,8,0,7,0,6,3,11,0,11,6,0,-1,-1,-1,-1},
    {7,11,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {7,6,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,0,8,11,7,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,1,9,11,7,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {8,1,9,8,3,1,11,7,6,-1,-1,-1,-1,-1,-1,-1},
    {10,1,2,6,11,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,3,0,8,6,11,7,-1,-1,-1,-1,-1,-1,-1},
    {2,9,0,2,10,9,6,11,7,-1,-1,-1,-1,-1,-1,-1},
    {6,11,7,2,10,3,10,8,3,10,9,8,-1,-1,-1,-1},
    {7,2,3,6,2,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {7,0,8,7,6,0,6,2,0,-1,-1,-1,-1,-1,-1,-1},
    {2,7,6,2,3,7,0,1,9,-1,-1,-1,-1,-1,-1,-1},
    {1,6,2,1,8,6,1,9,8,8,7,6,-1,-1,-1,-1},
    {10,7,6,10,1,7,1,3,7,-1,-1,-1,-1,-1,-1,-1},
    {10,7,6,1,7,10,1,8,7,1,0,8,-1,-1,-1,-1},
    {0,3,7,0,7,10,0,10,9,6,10,7,-1,-1,-1,-1},
    {7,6,10,7,10,8,8,10,9,-1,-1,-1,-1,-1,-1,-1},
    {6,8,4,11,8,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,6,11,3,0,6,0,4,6,-1,-1,-1,-1,-1,-1,-1},
    {8,6,11,8,4,6,9,0,1,-1,-1,-1,-1,-1,-1,-1},
    {9,4,6,9,6,3,9,3,1,11,3,6,-1,-1,-1,-1},
    {6,8,4,6,11,8,2,10,1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,3,0,11,0,6,11,0,4,6,-1,-1,-1,-1},
    {4,11,8,4,6,11,0,2,9,2,10,9,-1,-1,-1,-1},
    {10,9,3,10,3,2,9,4,3,11,3,6,4,6,3,-1},
    {8,2,3,8,4,2,4,6,2,-1,-1,-1,-1,-1,-1,-1},
    {0,4,2,4,6,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,9,0,2,3,4,2,4,6,4,3,8,-1,-1,-1,-1},
    {1,9,4,1,4,2,2,4,6,-1,-1,-1,-1,-1,-1,-1},
    {8,1,3,8,6,1,8,4,6,6,10,1,-1,-1,-1,-1},
    {10,1,0,10,0,6,6,0,4,-1,-1,-1,-1,-1,-1,-1},
    {4,6,3,4,3,8,6,10,3,0,3,9,10,9,3,-1},
    {10,9,4,6,10,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,9,5,7,6,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,4,9,5,11,7,6,-1,-1,-1,-1,-1,-1,-1},
    {5,0,1,5,4,0,7,6,11,-1,-1,-1,-1,-1,-1,-1},
    {11,7,6,8,3,4,3,5,4,3,1,5,-1,-1,-1,-1},
    {9,5,4,10,1,2,7,6,11,-1,-1,-1,-1,-1,-1,-1},
    {6,11,7,1,2,10,0,8,3,4,9,5,-1,-1,-1,-1},
    {7,6,11,5,4,10,4,2,10,4,0,2,-1,-1,-1,-1},
    {3,4,8,3,5,4,3,2,5,10,5,2,11,7,6,-1},
    {7,2,3,7,6,2,5,4,9,-1,-1,-1,-1,-1,-1,-1},
    {9,5,4,0,8,6,0,6,2,6,8,7,-1,-1,-1,-1},
    {3,6,2,3,7,6,1,5,0,5,4,0,-1,-1,-1,-1},
    {6,2,8,6,8,7,2,1,8,4,8,5,1,5,8,-1},
    {9,5,4,10,1,6,1,7,6,1,3,7,-1,-1,-1,-1},
    {1,6,10,1,7,6,1,0,7,8,7,0,9,5,4,-1},
    {4,0,10,4,10,5,0,3,10,6,10,7,3,7,10,-1},
    {7,6,10,7,10,8,5,4,10,4,8,10,-1,-1,-1,-1},
    {6,9,5,6,11,9,11,8,9,-1,-1,-1,-1,-1,-1,-1},
    {3,6,11,0,6,3,0,5,6,0,9,5,-1,-1,-1,-1},
    {0,11,8,0,5,11,0,1,5,5,6,11,-1,-1,-1,-1},
    {6,11,3,6,3,5,5,3,1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,9,5,11,9,11,8,11,5,6,-1,-1,-1,-1},
    {0,11,3,0,6,11,0,9,6,5,6,9,1,2,10,-1},
    {11,8,5,11,5,6,8,0,5,10,5,2,0,2,5,-1},
    {6,11,3,6,3,5,2,10,3,10,5,3,-1,-1,-1,-1},
    {5,8,9,5,2,8,5,6,2,3,8,2,-1,-1,-1,-1},
    {9,5,6,9,6,0,0,6,2,-1,-1,-1,-1,-1,-1,-1},
    {1,5,8,1,8,0,5,6,8,3,8,2,6,2,8,-1},
    {1,5,6,2,1,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,3,6,1,6,10,3,8,6,5,6,9,8,9,6,-1},
    {10,1,0,10,0,6,9,5,0,5,6,0,-1,-1,-1,-1},
    {0,3,8,5,6,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {10,5,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {11,5,10,7,5,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {11,5,10,11,7,5,8,3,0,-1,-1,-1,-1,-1,-1,-1},
    {5,11,7,5,10,11,1,9,0,-1,-1,-1,-1,-1,-1,-1},
    {10,7,5,10,11,7,9,8,1,8,3,1,-1,-1,-1,-1},
    {11,1,2,11,7,1,7,5,1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,1,2,7,1,7,5,7,2,11,-1,-1,-1,-1},
    {9,7,5,9,2,7,9,0,2,2,11,7,-1,-1,-1,-1},
    {7,5,2,7,2,11,5,9,2,3,2,8,9,8,2,-1},
    {2,5,10,2,3,5,3,7,5,-1,-1,-1,-1,-1,-1,-1},
    {8,2,0,8,5,2,8,7,5,10,2,5,-1,-1,-1,-1},
    {9,0,1,5,10,3,5,3,7,3,10,2,-1,-1,-1,-1},
    {9,8,2,9,2,1,8,7,2,10,2,5,7,5,2,-1},
    {1,3,5,3,7,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,7,0,7,1,1,7,5,-1,-1,-1,-1,-1,-1,-1},
    {9,0,3,9,3,5,5,3,7,-1,-1,-1,-1,-1,-1,-1},
    {9,8,7,5,9,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {5,8,4,5,10,8,10,11,8,-1,-1,-1,-1,-1,-1,-1},
    {5,0,4,5,11,0,5,10,11,11,3,0,-1,-1,-1,-1},
    {0,1,9,8,4,10,8,10,11,10,4,5,-1,-1,-1,-1},
    {10,11,4,10,4,5,11,3,4,9,4,1,3,1,4,-1},
    {2,5,1,2,8,5,2,11,8,4,5,8,-1,-1,-1,-1},
    {0,4,11,0,11,3,4,5,11,2,11,1,5,1,11,-1},
    {0,2,5,0,5,9,2,11,5,4,5,8,11,8,5,-1},
    {9,4,5,2,11,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,5,10,3,5,2,3,4,5,3,8,4,-1,-1,-1,-1},
    {5,10,2,5,2,4,4,2,0,-1,-1,-1,-1,-1,-1,-1},
    {3,10,2,3,5,10,3,8,5,4,5,8,0,1,9,-1},
    {5,10,2,5,2,4,1,9,2,9,4,2,-1,-1,-1,-1},
    {8,4,5,8,5,3,3,5,1,-1,-1,-1,-1,-1,-1,-1},
    {0,4,5,1,0,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {8,4,5,8,5,3,9,0,5,0,3,5,-1,-1,-1,-1},
    {9,4,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,11,7,4,9,11,9,10,11,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,4,9,7,9,11,7,9,10,11,-1,-1,-1,-1},
    {1,10,11,1,11,4,1,4,0,7,4,11,-1,-1,-1,-1},
    {3,1,4,3,4,8,1,10,4,7,4,11,10,11,4,-1},
    {4,11,7,9,11,4,9,2,11,9,1,2,-1,-1,-1,-1},
    {9,7,4,9,11,7,9,1,11,2,11,1,0,8,3,-1},
    {11,7,4,11,4,2,2,4,0,-1,-1,-1,-1,-1,-1,-1},
    {11,7,4,11,4,2,8,3,4,3,2,4,-1,-1,-1,-1},
    {2,9,10,2,7,9,2,3,7,7,4,9,-1,-1,-1,-1},
    {9,10,7,9,7,4,10,2,7,8,7,0,2,0,7,-1},
    {3,7,10,3,10,2,7,4,10,1,10,0,4,0,10,-1},
    {1,10,2,8,7,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,9,1,4,1,7,7,1,3,-1,-1,-1,-1,-1,-1,-1},
    {4,9,1,4,1,7,0,8,1,8,7,1,-1,-1,-1,-1},
    {4,0,3,7,4,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,8,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,10,8,10,11,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,0,9,3,9,11,11,9,10,-1,-1,-1,-1,-1,-1,-1},
    {0,1,10,0,10,8,8,10,11,-1,-1,-1,-1,-1,-1,-1},
    {3,1,10,11,3,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,11,1,11,9,9,11,8,-1,-1,-1,-1,-1,-1,-1},
    {3,0,9,3,9,11,1,2,9,2,11,9,-1,-1,-1,-1},
    {0,2,11,8,0,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,2,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,3,8,2,8,10,10,8,9,-1,-1,-1,-1,-1,-1,-1},
    {9,10,2,0,9,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,3,8,2,8,10,0,1,8,1,10,8,-1,-1,-1,-1},
    {1,10,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,3,8,9,1,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,9,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,3,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
};

// per edge: the owning corner's offset (di, dj, dk) packed as di | dj << 1 | dk << 2, and the axis (0 = i, 1 = j, 2 = k)
__constant__ unsigned char kMcEdgeOwner[12] = {0, 4, 2, 0, 1, 5, 3, 1, 0, 4, 6, 2};
__constant__ unsigned char kMcEdgeAxis[12] = {2, 1, 2, 1, 2, 1, 2, 1, 0, 0, 0, 0};

struct MeshArgs {
    const float* vol;                  // [nx][ny][nz] float32, C order
    int nx, ny, nz, n;                 // n = nx * ny * nz (< 2^31 / 3: every index below fits 32 bits)
    int nblk;                          // ceil(n / kMeshWG)
    float level;
    unsigned char* emask;              // [n]   bit a: the point's +axis-a edge crosses the level   (count -> emit)
    int* firstv;                       // [n]   the vertex id of the point's first crossing edge    (emit_vertices -> emit_faces)
    long long* blk;                    // [nblk][2] per-workgroup (vertices, faces): totals (count), exclusive offsets (scan)
    long long* counts;                 // [2]   totals (scan)
    float* verts; float* normals;      // [n_vertices][3]; normals may be null
    int* faces;                        // [n_faces][3]
    long long n_vertices, n_faces;     // capacities: nothing is written at or past them
    float A[12];                       // output affine, rows [A | b] (has_affine), applied to the index-space vertex
    float Ninv[9];                     // inverse transpose of A's linear part (rows), for the normals
    int has_affine;
    const unsigned char* valid;        // [n] non-zero = the point holds a value; null (a zero-filled MeshArgs) = no mask
    int* edge_ids;                     // [n_vertices] owning point * 3 + axis of every vertex; may be null
};

__device__ __forceinline__ void decode(int p, const MeshArgs& a, int& i, int& j, int& k) {
    k = p % a.nz;
    const int r = p / a.nz;
    j = r % a.ny;
    i = r / a.ny;
}

__device__ __forceinline__ unsigned cube_index(const MeshArgs& a, int p) {
    const int si = a.ny * a.nz, sj = a.nz;
    const float* v = a.vol + p;
    const float lv = a.level;
    return (unsigned)(v[0] > lv) | (unsigned)(v[1] > lv) << 1 | (unsigned)(v[sj + 1] > lv) << 2 | (unsigned)(v[sj] > lv) << 3 |
           (unsigned)(v[si] > lv) << 4 | (unsigned)(v[si + 1] > lv) << 5 | (unsigned)(v[si + sj + 1] > lv) << 6 |
           (unsigned)(v[si + sj] > lv) << 7;
}

__device__ __forceinline__ int tri_count(unsigned cube) {
    int n = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) n += kMcTri[cube][3 * t] >= 0;
    return n;
}

// the cell whose lowest corner is p exists iff p is not on an upper face of the grid
__device__ __forceinline__ bool owns_cell(const MeshArgs& a, int i, int j, int k) {
    return i + 1 < a.nx && j + 1 < a.ny && k + 1 < a.nz;
}

// The mask (a.valid != null).  A cell exists iff, besides, all eight corners are valid; faces come from existing cells only; the
// crossing on a grid edge becomes a vertex iff at least one of the up to four cells around the edge exists, so that no vertex is left
// unreferenced.  With every point valid all of this is the unmasked rule (every side of the grid is >= 2: an edge always has a cell).
__device__ __forceinline__ bool corners_valid(const MeshArgs& a, int p) {
    const int si = a.ny * a.nz, sj = a.nz;
    const unsigned char* v = a.valid + p;
    return v[0] && v[1] && v[sj + 1] && v[sj] && v[si] && v[si + 1] && v[si + sj + 1] && v[si + sj];
}

__device__ __forceinline__ bool cell_exists(const MeshArgs& a, int p, int i, int j, int k) {
    return owns_cell(a, i, j, k) && (!a.valid || corners_valid(a, p));
}

// whether a cell around the +axis-ax edge of point p = (idx) exists: the cells whose lowest corner is p less 0 or 1 along each of the
// two other axes
__device__ __forceinline__ bool edge_has_cell(const MeshArgs& a, int p, const int idx[3], int ax) {
    const int stride[3] = {a.ny * a.nz, a.nz, 1};
    const int u = (ax + 1) % 3, w = (ax + 2) % 3;
    for (int bu = 0; bu < 2; ++bu)
        for (int bw = 0; bw < 2; ++bw) {
            int c[3] = {idx[0], idx[1], idx[2]};
            c[u] -= bu;
            c[w] -= bw;
            if (c[u] < 0 || c[w] < 0) continue;
            if (cell_exists(a, p - bu * stride[u] - bw * stride[w], c[0], c[1], c[2])) return true;
        }
    return false;
}

__global__ __launch_bounds__(kMeshWG) void mesh_count(const MeshArgs a) {
    __shared__ int lds4[2][kMeshWG / 64];
    const int p = blockIdx.x * kMeshWG + threadIdx.x;
    int nv = 0, nf = 0;
    if (p < a.n) {
        int i, j, k;
        decode(p, a, i, j, k);
        const float* v = a.vol + p;
        const bool up = v[0] > a.level;
        unsigned m = 0;
        if (i + 1 < a.nx) m |= (unsigned)((v[a.ny * a.nz] > a.level) != up);
        if (j + 1 < a.ny) m |= (unsigned)((v[a.nz] > a.level) != up) << 1;
        if (k + 1 < a.nz) m |= (unsigned)((v[1] > a.level) != up) << 2;
        if (a.valid && m) {            // crossings are sparse: the cells around an edge are looked at for those only
            const int idx[3] = {i, j, k};
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
                if ((m >> ax & 1u) && !edge_has_cell(a, p, idx, ax)) m &= ~(1u << ax);
        }
        a.emask[p] = (unsigned char)m;
        nv = __popc(m);
        if (cell_exists(a, p, i, j, k)) nf = tri_count(cube_index(a, p));
    }
    int tv, tf;                        // two scans in a row: an LDS array each (scan_ops.h's barrier contract)
    vscan::wg_exclusive_scan<kMeshWG>(nv, lds4[0], tv);
    vscan::wg_exclusive_scan<kMeshWG>(nf, lds4[1], tf);
    if (threadIdx.x == 0) {
        a.blk[2 * blockIdx.x] = tv;
        a.blk[2 * blockIdx.x + 1] = tf;
    }
}

// One workgroup: the per-workgroup totals -> exclusive offsets (in place), grand totals -> counts.  One pass over blk: vertices in
// the low and faces in the high half of one 64-bit word per workgroup.  No running sum leaves its half: vertices <= 3 n < 2^31 and
// faces <= 5 n < 2^32 (3 n < 2^31 is the C ABI's limit on the volume).
__global__ __launch_bounds__(kScanWG) void mesh_scan(const MeshArgs a) {
    __shared__ unsigned long long wsum[kScanWG / 64];
    const unsigned long long sum = vscan::wg_scan_totals<kScanWG>(
        a.nblk, wsum, [&](long long b) { return (unsigned long long)a.blk[2 * b] | (unsigned long long)a.blk[2 * b + 1] << 32; },
        [&](long long b, unsigned long long ex) {
            a.blk[2 * b] = (long long)(ex & 0xffffffffull);
            a.blk[2 * b + 1] = (long long)(ex >> 32);
        });
    if (threadIdx.x == 0) {
        a.counts[0] = (long long)(sum & 0xffffffffull);
        a.counts[1] = (long long)(sum >> 32);
    }
}

// numpy.gradient's stencil of the volume at point (i, j, k): central differences inside, one-sided (first order) at the borders.
// An invalid neighbour counts as the border; with neither side valid the component is 0 (without a mask every side of the grid is
// >= 2, so one side always exists).
__device__ __forceinline__ float grad_axis(const MeshArgs& a, int p, int at, int dim, int s) {
    const float* v = a.vol + p;
    const bool lo = at > 0 && (!a.valid || a.valid[p - s]), hi = at < dim - 1 && (!a.valid || a.valid[p + s]);
    return lo && hi ? (v[s] - v[-s]) * 0.5f : hi ? v[s] - v[0] : lo ? v[0] - v[-s] : 0.0f;
}

__device__ __forceinline__ void grad_at(const MeshArgs& a, int i, int j, int k, float g[3]) {
    const int p = (i * a.ny + j) * a.nz + k;
    g[0] = grad_axis(a, p, i, a.nx, a.ny * a.nz);
    g[1] = grad_axis(a, p, j, a.ny, a.nz);
    g[2] = grad_axis(a, p, k, a.nz, 1);
}

__global__ __launch_bounds__(kMeshWG) void mesh_emit_vertices(const MeshArgs a) {
    __shared__ int lds4[kMeshWG / 64];
    const int p = blockIdx.x * kMeshWG + threadIdx.x;
    const unsigned m = p < a.n ? a.emask[p] : 0u;
    int total;
    const int local = vscan::wg_exclusive_scan<kMeshWG>((int)__popc(m), lds4, total);
    if (m == 0) return;
    const long long v0id = a.blk[2 * blockIdx.x] + local;
    a.firstv[p] = (int)v0id;
    int idx[3];
    decode(p, a, idx[0], idx[1], idx[2]);
    const int stride[3] = {a.ny * a.nz, a.nz, 1};
    const float v0 = a.vol[p];
    float g0[3];
    if (a.normals) grad_at(a, idx[0], idx[1], idx[2], g0);
    long long vid = v0id;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (!(m >> ax & 1u)) continue;
        const float v1 = a.vol[p + stride[ax]];
        const float t = (a.level - v0) / (v1 - v0);
        float pos[3] = {(float)idx[0], (float)idx[1], (float)idx[2]};
        pos[ax] += t;
        if (vid < a.n_vertices) {
            if (a.edge_ids) a.edge_ids[vid] = 3 * p + ax;
            float* out = a.verts + 3 * vid;
            if (a.has_affine) {
#pragma unroll
                for (int r = 0; r < 3; ++r) out[r] = fmaf(a.A[4 * r + 2], pos[2], fmaf(a.A[4 * r + 1], pos[1], fmaf(a.A[4 * r], pos[0], a.A[4 * r + 3])));
            } else {
                out[0] = pos[0]; out[1] = pos[1]; out[2] = pos[2];
            }
            if (a.normals) {
                float g1[3];
                grad_at(a, idx[0] + (ax == 0), idx[1] + (ax == 1), idx[2] + (ax == 2), g1);
                float n[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) n[c] = -(g0[c] * (1.0f - t) + g1[c] * t);
                if (a.has_affine) {
                    float q[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r) q[r] = a.Ninv[3 * r] * n[0] + a.Ninv[3 * r + 1] * n[1] + a.Ninv[3 * r + 2] * n[2];
                    n[0] = q[0]; n[1] = q[1]; n[2] = q[2];
                }
                const float nn = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                const float inv = nn > 0.0f ? 1.0f / nn : 0.0f;
                float* on = a.normals + 3 * vid;
                on[0] = n[0] * inv; on[1] = n[1] * inv; on[2] = n[2] * inv;
            }
        }
        ++vid;
    }
}

__global__ __launch_bounds__(kMeshWG) void mesh_emit_faces(const MeshArgs a) {
    __shared__ int lds4[kMeshWG / 64];
    const int p = blockIdx.x * kMeshWG + threadIdx.x;
    unsigned cube = 0;
    int nt = 0;
    if (p < a.n) {
        int i, j, k;
        decode(p, a, i, j, k);
        if (cell_exists(a, p, i, j, k)) {
            cube = cube_index(a, p);
            nt = tri_count(cube);
        }
    }
    int total;
    const int local = vscan::wg_exclusive_scan<kMeshWG>(nt, lds4, total);
    if (nt == 0) return;
    const long long f0 = a.blk[2 * blockIdx.x + 1] + local;
    const int si = a.ny * a.nz, sj = a.nz;
    for (int t = 0; t < nt; ++t) {
        if (f0 + t >= a.n_faces) break;
        int* out = a.faces + 3 * (f0 + t);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int e = kMcTri[cube][3 * t + r];
            const unsigned o = kMcEdgeOwner[e];
            const int q = p + (int)(o & 1u) * si + (int)(o >> 1 & 1u) * sj + (int)(o >> 2);
            const unsigned ax = kMcEdgeAxis[e];
            out[r] = a.firstv[q] + __popc((unsigned)a.emask[q] & ((1u << ax) - 1u));
        }
    }
}

// The dense grid Trainer.meshing queries: point (i, j, k) -> A (i, j, k) + b, written as [n][3] float32 in C order.
__global__ __launch_bounds__(kMeshWG) void mesh_grid_points(const MeshArgs a, float* points) {
    const int p = blockIdx.x * kMeshWG + threadIdx.x;
    if (p >= a.n) return;
    int i, j, k;
    decode(p, a, i, j, k);
    const float x = (float)i, y = (float)j, z = (float)k;
    float* out = points + 3 * (long long)p;
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = fmaf(a.A[4 * r + 2], z, fmaf(a.A[4 * r + 1], y, fmaf(a.A[4 * r], x, a.A[4 * r + 3])));
}

}  // namespace vm
