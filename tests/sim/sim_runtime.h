// sim_runtime.h - TEST INFRASTRUCTURE: a tiny SIMT executor for running the HIP kernel *source* on a CPU.
//
// Workgroups are independent and dealt to a few OS threads; inside a workgroup every work-item is a ucontext fiber
// scheduled on ONE thread, cooperative (no preemption), fully deterministic.  Schedule 0 (the default) is round-robin over all
// fibers; schedules 1 / 2 are wave-greedy, forward / reverse (set_schedule below): waves run ahead of each other as they do on hardware.  A wave is 64 consecutive fibers; wave-collective
// operations (the matrix instruction, lane exchanges) and barriers are rendezvous points at which a
// fiber yields until all participants have arrived.  LDS is a per-block byte array filled with
// signalling garbage (NaN patterns) so that reads of unwritten shared memory surface as NaNs.
//
// This models the *interface* documented in vmap_amd/csrc/wave_ops.h (operand/accumulator lane maps of
// v_mfma_f32_32x32x2_f32 from /opt/skills/guides/cdna_hip_programming.md section 3); it does not model timing.
#pragma once
#include <ucontext.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

namespace sim {

struct Idx3 { unsigned x, y, z; };

struct Barrier { int n = 0, count = 0; unsigned gen = 0; };

constexpr int kWave = 64;
constexpr int kMaxWaves = 16;

struct Fiber {
    ucontext_t ctx;
    char* stack = nullptr;
    bool done = false;
    unsigned tid = 0;
    unsigned shfl_turn = 0;          // which of Block::x8's two buffers this lane's next __shfl_up uses
    bool at_block_bar = false;       // waiting at the workgroup barrier for generation block_gen to end (the wave-greedy schedules)
    unsigned block_gen = 0;
};

struct Block {
    int nthreads = 0;
    std::vector<Fiber> fibers;
    Barrier block_bar;
    Barrier wave_bar[kMaxWaves];
    float xa[kMaxWaves][kWave];
    float xb[kMaxWaves][kWave];
    unsigned xa4[kMaxWaves][kWave][4];      // bf16 matrix-instruction operands (four dwords per lane)
    unsigned xb4[kMaxWaves][kWave][4];
    const void* xp[kMaxWaves][kWave];       // per-lane addresses of a transposing LDS read
    unsigned long long x8[2][kMaxWaves][kWave];   // __shfl_up: 4- and 8-byte values, two buffers used in turn
    std::vector<unsigned char> lds;
};

extern thread_local Block* g_block;
extern thread_local Fiber* g_cur;
extern thread_local ucontext_t g_sched;
extern thread_local Idx3 g_blockIdx;
extern Idx3 g_gridDim, g_blockDim;
extern thread_local long g_yields;

inline void yield() {
    ++g_yields;
    swapcontext(&g_cur->ctx, &g_sched);
}

inline void barrier_wait(Barrier& b) {
    unsigned gen = b.gen;
    if (++b.count == b.n) {
        b.count = 0;
        ++b.gen;
    } else {
        while (b.gen == gen) yield();
    }
}

inline unsigned tid() { return g_cur->tid; }
inline int wave_id() { return (int)(g_cur->tid / kWave); }
inline int lane_id() { return (int)(g_cur->tid % kWave); }
inline void wave_barrier() { barrier_wait(g_block->wave_bar[wave_id()]); }

// the workgroup barrier: like barrier_wait, and it tells the scheduler that this fiber cannot run before the generation ends
inline void block_barrier() {
    Barrier& b = g_block->block_bar;
    const unsigned gen = b.gen;
    if (++b.count == b.n) {
        b.count = 0;
        ++b.gen;
    } else {
        g_cur->at_block_bar = true;
        g_cur->block_gen = gen;
        while (b.gen == gen) yield();
        g_cur->at_block_bar = false;
    }
}

void launch(unsigned grid, unsigned block, size_t lds_bytes, const std::function<void()>& body);
// a 3-D grid: workgroup (x, y, z) is flat index x + gx * (y + gy * z); launch(grid, ...) is launch3(grid, 1, 1, ...)
void launch3(unsigned gx, unsigned gy, unsigned gz, unsigned block, size_t lds_bytes, const std::function<void()>& body);

// The order in which the fibers of a workgroup are run.  0: round-robin over all fibers, each up to its next rendezvous - every wave
// leaves a barrier in the same sweep, so no wave ever runs ahead of another.  1 / 2: wave-greedy - one wave runs until each of its
// fibers is done or waits at the WORKGROUP barrier, then the next wave (1: waves 0, 1, 2 ...; 2: the last wave first).  The wave that
// arrives last at a workgroup barrier goes straight on to the next one while the others still stand at the first: a missing barrier
// between two uses of the same shared memory shows.  It orders whole waves only; lanes of one wave still move in step.
void set_schedule(int s);

}  // namespace sim
