// group.h -- what the translation units of the multi-GPU paths share
// (exchange.cpp, group.cpp, group_blocks.cpp): the one-process group of
// replicas and the few functions that cross those files.  Internal, like
// train_host.h: not part of the installed interface.
#pragma once
#include <rccl/rccl.h>

#include <string>
#include <vector>

#include "comm_watch.h"
#include "ctx.h"

struct smore_group {
    std::vector<smore_ctx*> ctx;
    std::vector<ncclComm_t> comms;
    std::string err;
    // hub-row exchange (smore_group_set_hot_exchange): rows per table (-1:
    // automatic, 0: off) and training launches per exchange round
    int64_t hot_rows = -1;
    int launches = 8;
    double c0 = -1.0;   // adaptive exchange (smore_group_set_adaptive); -1: 2048 with the source partition, else 64
    int partition = 1;  // LINE-2: W rows partitioned by source (smore_group_set_partition)
    int walk_partition = 0;   // walk models: W rows partitioned by walk center (smore_group_set_walk_partition)
    // every replica on one device: collectives as device passes, ordered by
    // events between the replicas' streams (no RCCL)
    bool local = false;
    std::vector<hipEvent_t> lev;   // one per replica
    hipEvent_t ldone = nullptr;
    // the 2-D block schedule (smore_group_set_schedule): per replica the
    // compute-done event of a sub-round and the receive-done events of the
    // last two rotations (by sub-round parity)
    int schedule = SMORE_SCHED_BLOCKS;   // include/smore_hip.h: the default
    std::vector<hipEvent_t> bdone, brecv;
    // the block schedule's hub slots (blocks.cpp): per replica the event
    // after its exchange pass (compute stream) and after the all-reduce
    std::vector<hipEvent_t> hready, hdone;
    // same-device studies (SMORE_LOCAL_SERIAL=1): the replicas' cells run one
    // after another, each with the whole GPU as on its own device
    std::vector<hipEvent_t> lser;
};

namespace smore_host {

inline int gfail(smore_group* g, int rank, int rc) {
    if (g && rc != SMORE_OK && rank >= 0) g->err = "replica " + std::to_string(rank) + ": " + g->ctx[rank]->err;
    return rc;
}

// ---------------------------------------------------------------- exchange.cpp
// the RCCL table (comm_watch.h): loaded on first use; nullptr when unavailable
Rccl* rccl();
int nccl_fail(smore_ctx* c, const char* what, ncclResult_t r);
double comm_timeout();
size_t table_floats(const smore_ctx* c);
// one context's side of a replica exchange (the group adds the collective)
int exchange_reset(smore_ctx* c);
int exchange_passes(smore_ctx* c, int mode);
int exchange_posted(smore_ctx* c);
int exchange_end(smore_ctx* c);
int adaptive_scales(smore_ctx* c, int model, int K, double updates, double c0, int nranks,
                    std::vector<float> (&out)[2]);
int upload_scales(smore_ctx* c, const std::vector<float> (&sc)[2], const std::string& key);
std::string scale_key(int model, int K, double updates, double c0, int nranks, const smore_ctx* c);

// ---------------------------------------------------------------- group.cpp
int coll_allreduce(smore_group* g, const std::vector<float*>& buf, size_t n, const std::vector<hipStream_t>& st,
                   const char* what);
int coll_broadcast(smore_group* g, const std::vector<float*>& buf, size_t n, int root,
                   const std::vector<hipStream_t>& st, const char* what);
std::vector<hipStream_t> compute_streams(const smore_group* g);
int group_sync(smore_group* g);

// ---------------------------------------------------------------- group_blocks.cpp
// the block schedule's drivers of a group call (LINE-2; DeepWalk / Walklets)
int group_block_edges(smore_group* g, uint64_t begin, uint64_t count, uint64_t per, uint64_t total, int K,
                      double alpha0, uint64_t seed, int mode);
int group_block_walks(smore_group* g, int rule, uint64_t walk_begin, uint64_t walk_end, int walk_times,
                      int walk_steps, int window, int window_min, int K, double alpha0, uint64_t seed,
                      const int64_t* order, int mode, uint64_t per);

}  // namespace smore_host
