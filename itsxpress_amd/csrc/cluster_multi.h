// cluster_multi.h -- greedy clustering of one sample with the centroid stream spread over several contexts (itsx_cluster_multi).
//
// The leader runs cluster_run as ever; the only quadratic step, streaming every existing centroid past the window's query strands
// (k_cl_stream mode 1), is split by centroid column over SHARDS: shard 0 on the leader, shard h on the h-th helper context.  Each
// shard keeps the 32 best rank keys of every strand over its own columns; the global 32 best are the 32 best of the union of the
// shards' lists, because the rank key is a total order (cluster_multi.hip explains why a shard's thresholds keep that exact).
#pragma once
#include <memory>
#include <string>
#include <vector>
#include "engine.h"
#include "k_api.h"

namespace itsx {

struct ShardSet;

class ClusterShards {
 public:
  struct Helper { int device; hipStream_t st; };
  ClusterShards(int leader_device, hipStream_t leader_st, const std::vector<Helper> &helpers);
  ~ClusterShards();                                          // waits for the helpers' streams, then frees every shard buffer
  // before the first window: the run's sizes (a.kcap, a.hcap, a.heavy_min, a.strand_both; nqs = strands of the largest window)
  hipError_t init(const ClusterArgs &a, int32_t nqs, int64_t n_kept, int64_t pool_cap);
  // the window's candidate lists (replaces the mode-1 stream loop): the leader's query index is built; afterwards the leader's lists
  // hold shard 0's and every helper's <= 32 keys per strand, ready for k_cl_topk(..., 1)
  hipError_t stream(const ClusterArgs &a, int64_t &launches);
  // queued on the leader's stream before the window's last synchronisation: the metadata of columns [c0, c0 + a.nq) to the host
  hipError_t fetch_columns(const ClusterArgs &a, int32_t c0);
  // after a window that is kept: columns [c0, c0 + consumed) are final; each shard adopts the ones it owns
  hipError_t adopt(const ClusterArgs &a, int32_t c0, int32_t consumed);
  void sync();                                               // waits for every helper stream
  int shards() const;
  std::string debug_line(int64_t windows) const;
  const std::string &error() const { return err_; }

 private:
  std::unique_ptr<ShardSet> s_;
  std::string err_;
};

}  // namespace itsx
