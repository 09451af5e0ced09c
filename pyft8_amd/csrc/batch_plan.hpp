// batch_plan.hpp -- how a batch of B frames is cut into chunks and how the chunks' kernel chains are ordered: the partition rule
// of ft8rx.hip's launch_batch as a pure function.  No HIP: compiles with plain g++ (tests/host_asan_driver.cpp checks it).
#pragma once
#include <stdint.h>

namespace batchplan {

enum { MAX_STREAMS = 8, MAX_CHUNKS = 2 * MAX_STREAMS };      // ft8rx_set_streams' limit; the handle's per-chunk arrays hold MAX_CHUNKS
enum Entry { DEVICE, HOST_SYNC, HOST_PIPELINED };            // ft8rx_enqueue_batch / ft8rx_decode_batch / ft8rx_enqueue_batch_host
enum Mode { SINGLE, FORK_JOIN, FREE_RUN };
// chunk k = frames [cb[k], cb[k + 1]) on stream k % n_streams; SINGLE: one chunk, the whole batch on the main stream
struct BatchPlan { Mode mode; int nc; int cb[MAX_CHUNKS + 1]; };

inline BatchPlan plan_batch(int B, int n_streams, bool profiling, Entry e) {
    BatchPlan p;
    // profiling mode / small batches: one chain on the main stream (per-stage events bracket whole-batch launches);
    // otherwise the batch is cut into chunks whose chains overlap on the sub-streams -- the ladder kernels (BP, OSD, fine sync)
    // are latency bound, so chunks fill each other's stalls.
    // synchronous host entry: twice as many chunks, so that the first kernels start after 1/8 of the copy; the pipelined entry's copies
    // already overlap the previous batch, so it keeps the 4 larger chunks of the device-resident path
    int nc = profiling ? 1 : (e == HOST_SYNC ? 2 * n_streams : n_streams);
    if (nc > B / 8) nc = B / 8;
    // Chunk k runs on stream k % n_streams, where stream 0 IS the handle's main stream and streams 1.. are the (lazily created)
    // sub-streams.  The HIP runtime maps all streams of a process onto four hardware queues, and commands of streams that share
    // one execute in submission order: with a main stream that only forks and joins plus two chunk streams plus the two copy
    // streams (five), the H2D stream shared a queue with a chunk stream and its event markers waited behind that chunk's kernels --
    // in the rocprofv3 trace the second H2D chunk of the pipelined host entry started only when the previous batch's last kernel
    // had finished (profiles/archive/r03_notes.md).  Four streams in use = a queue each.
    //
    // Free-running chunk streams: with the audio resident (or staged by the pipelined host entry) and one chunk per stream, chunk i of
    // batch k+1 simply follows chunk i of batch k on stream i.  Every workspace is indexed by frame, so a stream only ever touches
    // its own frame range and in-stream order is all the ordering the chains need; only the result copy waits for all of them.
    // Without the per-batch fork / join a stream that finishes its half early starts on the next batch while the other one is still
    // in its tail.  Anything else that uses the workspaces (stage entry points, the synchronous entry, a different partition)
    // goes through quiesce() / need_barrier.
    // (A/B on one box, profiles/archive/r03_notes.md: 48 498 -> 49 001 frames/s end to end, 48 167 -> 48 894 including H2D.)
    p.mode = nc <= 1 ? SINGLE : (!profiling && nc == n_streams && e != HOST_SYNC) ? FREE_RUN : FORK_JOIN;
    p.nc = nc = nc < 1 ? 1 : nc;
    // chunk boundaries: equal parts, except for the synchronous host entry, whose first kernels can only start when the first
    // chunk's audio has crossed PCIe -- there the chunks grow geometrically (B/8, B/8, B/4, B/2 for four): the first copy is
    // half as long and the large chunks, which run most efficiently, come last (38.8 k -> 40.5 k frames/s for 256-frame calls;
    // other layouts -- 16/48/64/128, three streams, five or six chunks -- all land between 38 k and 41.5 k)
    const int per = (B + nc - 1) / nc;
    for (int k = 0; k <= MAX_CHUNKS; k++) p.cb[k] = (k < nc && k * per < B) ? k * per : B;
    if (e == HOST_SYNC && nc >= 3 && B >= 8 * nc) {
        // (kept as it is: from ten chunks on some come out empty or one frame long, 129 frames on 8 streams = 0 1 1 .. 1 2 3 5 9 .. 129)
        int left = B;
        for (int k = nc - 1; k >= 1; k--) { const int n = left / 2; p.cb[k] = left - n; left -= n; }
    }
    return p;
}

}  // namespace batchplan
