// queue.cc -- arch5's batch queue (engine.h): the slots in shared host memory, their ticket protocol, and its two
// ends -- a sampler process's SendOne, a trainer process's Receive + Unpack.  Citations are relative to the reference's
// samgraph/common/.
//
// MemoryQueue (dist/memory_queue.cc) + DistEngine's queue set-up (dist_engine.cc:395-397).  The reference serialises a
// Task into a queue slot with host copies and a mutex-guarded ring; here the sampler's GPU writes the batch into the
// slot itself (ggms_queue_pack: one launch, every length read on the device) and the trainer's GPU reads it out
// (ggms_queue_unpack), and the ring is lock-free: tickets from two counters, one sequence word per slot.
#include "engine.h"

#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <string>

namespace sam {

// the first page of the queue's mapping, zeroed by the anonymous mapping (see QueueInit)
struct Engine::QueueCtl {
  alignas(64) uint64_t enqueue_pos; // next producer ticket
  alignas(64) uint64_t dequeue_pos; // next consumer ticket
  alignas(64) uint64_t ranking_ready; // pre_sample: sampler 0 has written ds.ranking_nodes
};

// the parent, before the fork: no GPU is touched (every process registers the slots itself, QueueMap)
void Engine::QueueInit() {
  static_assert(sizeof(QueueCtl) <= 4096, "the control block fits its page");
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t L = (uint32_t)cfg.fanout.size();
  SAM_CHECK(L <= GGMS_QUEUE_MAX_LAYERS, "arch5: at most GGMS_QUEUE_MAX_LAYERS layers");
  SAM_GGMS(ggms_queue_layout(&qlay_, L, max_edges_.data(), max_unique_, max_seeds_, cfg.sample_type == GGMS_RANDOM_WALK));
  queue_depth_ = cfg.queue_depth;
  const size_t bytes = 4096 + queue_depth_ * qlay_.slot_bytes;
  void *m = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
  SAM_CHECK(m != MAP_FAILED, "arch5: batch queue mmap of " + std::to_string(bytes) + " bytes failed");
  queue_ = (QueueCtl *)m;
  queue_slots_ = (char *)m + 4096;
  for (size_t i = 0; i < queue_depth_; ++i) __atomic_store_n(&QueueHeader(i)->seq, (uint64_t)i, __ATOMIC_RELAXED);
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  prof.LogInit(/*kLogInitL2DistQueue*/ 7, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  log_info("arch5: batch queue of " + std::to_string(queue_depth_) + " slots x " + std::to_string(qlay_.slot_bytes) + " bytes");
}

// this process's device reads / writes the slots in place: pinned and mapped (cudaHostRegister, dist_engine.cc:217-241)
void Engine::QueueMap() {
  SAM_HIP(hipHostRegister(queue_slots_, queue_depth_ * qlay_.slot_bytes, hipHostRegisterMapped));
  void *d = nullptr;
  SAM_HIP(hipHostGetDevicePointer(&d, queue_slots_, 0));
  queue_slots_dev_ = (char *)d;
}

ggms_queue_header_t *Engine::QueueHeader(uint64_t pos) const {
  return (ggms_queue_header_t *)(queue_slots_ + (pos % queue_depth_) * qlay_.slot_bytes);
}

// Every wait on another process has a deadline (queue_timeout_s): a sampler or trainer that died, or that stopped
// early, must not hold the others.  The process then ends with status 1 -- nothing in it is at fault, there is nothing
// to dump.  false: the engine is shutting down (a background loop waiting for a message that will not come).
bool Engine::QueueWait(const uint64_t *word, uint64_t want, const char *what, bool stoppable) {
  const auto t0 = std::chrono::steady_clock::now();
  for (uint64_t spin = 0;; ++spin) {
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return true;
    if (spin < 4096) continue;
    if (stoppable && bg_stop_.load()) return false;
    if ((spin & 63) == 0) {
      const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (waited > cfg.queue_timeout_s) {
        std::fprintf(stderr, "[samgraph-amd FATAL] %s:%d: arch5: %s %d (device %d) waited %d s for %s -- queue_timeout_s "
                             "= %g s passed; a process on the other side died, stopped early or is stuck\n",
                     __FILE__, __LINE__, role_ == kRoleSampler ? "sampler" : "trainer", worker_id_, device_, (int)waited,
                     what, cfg.queue_timeout_s);
        std::fflush(stderr);
        _exit(1);
      }
    }
    spin < 65536 ? (void)sched_yield() : (void)usleep(100);
  }
}

// pre_sample: sampler 0 publishes its ranking (ds.ranking_nodes, shared pages); the other samplers and the trainers
// wait for it (dist_engine.cc:451-466)
void Engine::PublishRanking() { __atomic_store_n(&queue_->ranking_ready, (uint64_t)1, __ATOMIC_RELEASE); }
void Engine::WaitRankingReady() { QueueWait(&queue_->ranking_ready, 1, "sampler 0's presample ranking", false); }

// train_init of an arch5 trainer: its GPU, its extract streams, its share of each epoch's messages, the slots
void Engine::Arch5TrainerInit(int worker_id, const std::string &ctx) {
  SAM_CHECK(data_ready_, "samgraph_data_init first");
  SAM_CHECK(role_ == kRoleNone, "arch5: a process is one sampler or one trainer (one sample_init or one train_init)");
  SAM_CHECK(worker_id >= 0 && (size_t)worker_id < cfg.num_train_worker, "arch5: train_init(worker_id) with 0 <= "
            "worker_id < num_train_worker = " + std::to_string(cfg.num_train_worker));
  role_ = kRoleTrainer;
  worker_id_ = worker_id;
  device_ = trainer_device_ = parse_device(ctx);
  SAM_HIP(hipSetDevice(device_));
  SAM_HIP(hipStreamCreateWithFlags(&stream_extract_, hipStreamNonBlocking));
  if (cfg.extract_streams > 1) SAM_HIP(hipStreamCreateWithFlags(&stream_extract2_, hipStreamNonBlocking));
  // the scripts' split of an epoch's steps over the trainers (multi_gpu/train_graphsage.py: steps w, w + T, ...)
  const size_t T = cfg.num_train_worker;
  num_local_step_ = num_global_step_ / T + ((size_t)worker_id < num_global_step_ % T ? 1 : 0);
  prof.Resize(cfg.num_epoch, num_global_step_);
  if (cfg.UsePresample()) WaitRankingReady(); // the cache is built from sampler 0's ranking
  QueueMap();
  sample_ready_ = true; // (the bounds are the parent's, ComputeBounds in DataInit)
}

// RunSampleSubLoopOnce (dist_loops_arch5.cc): shuffle, sample, send.  The reference's DoGetCacheMissIndex is not run:
// the trainer's gather resolves hits itself, and a hit / miss split would only add bytes to the message.
void Engine::SendOne() {
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
  SAM_HIP(hipSetDevice(device_));
  const uint32_t L = (uint32_t)cfg.fanout.size();
  Batch *b = sbatch_.get();
  hipStream_t ss = stream_;
  const auto t0 = clk::now();
  if (!ShufflerNext(b, ss))
    fatal(__FILE__, __LINE__, "arch5: sample_once() on sampler " + std::to_string(worker_id_) + " after its last batch (" +
                                  std::to_string(cfg.num_epoch) + " epochs x " + std::to_string(num_local_step_) +
                                  " steps, num_local_step())");
  const double t_shuffle = since(t0);
  SampleInto(b, pipes_[0]); // (pipeline 0: stream_)
  SAM_HIP(hipEventSynchronize(b->ev_sampled)); // DoGPUSample ends with a stream sync too
  const double t_sample = since(t0);
  // send: a free slot (the ticket's), the pack, its completion, then the slot is published
  const auto t1 = clk::now();
  const uint64_t pos = __atomic_fetch_add(&queue_->enqueue_pos, 1, __ATOMIC_ACQ_REL);
  ggms_queue_header_t *h = QueueHeader(pos);
  const std::string what = "a free queue slot from the trainers (ticket " + std::to_string(pos) + ")";
  QueueWait(&h->seq, pos, what.c_str(), false);
  const ggms_queue_batch_t src = b->sampler.View();
  SAM_GGMS(ggms_queue_pack(queue_slots_dev_ + (pos % queue_depth_) * qlay_.slot_bytes, &qlay_, &src, b->key, b->num_seeds, ss));
  SAM_HIP(hipEventRecord(b->ev_done, ss));
  SAM_HIP(hipEventSynchronize(b->ev_done));
  const uint64_t status = h->counts[GGMS_COUNT_STATUS(L)], num_input = h->counts[GGMS_COUNT_INPUT(L)];
  uint64_t edges = 0;
  for (uint32_t i = 0; i < L; ++i) edges += h->counts[GGMS_COUNT_EDGES(i)];
  CheckBatchStatus(status, b->key);
  __atomic_store_n(&h->seq, pos + 1, __ATOMIC_RELEASE); // published
  const double t_send = since(t1);
  // the items the multi_gpu scripts read (dist_loops_arch5.cc:95-107); no cache-miss split here, so its item is 0
  prof.LogEpochAdd(b->key, 0 /*kLogEpochSampleTime*/, t_sample);
  prof.LogEpochAdd(b->key, 1 /*KLogEpochSampleGetCacheMissIndexTime*/, 0.0);
  prof.LogEpochAdd(b->key, 2 /*kLogEpochSampleSendTime*/, t_send);
  prof.LogEpochAdd(b->key, 3 /*kLogEpochSampleTotalTime*/, t_sample + t_send);
  prof.LogEpochAdd(b->key, 15 /*kLogEpochNumSample*/, (double)edges);
  prof.LogStep(b->key, 0 /*kLogL1NumSample*/, (double)edges);
  prof.LogStep(b->key, 1 /*kLogL1NumNode*/, (double)num_input);
  prof.LogStep(b->key, 3 /*kLogL1SampleTime*/, t_sample);
  prof.LogStep(b->key, 4 /*kLogL1SendTime*/, t_send);
  prof.LogStep(b->key, 17 /*kLogL2ShuffleTime*/, t_shuffle);
}

// RunCacheDataCopySubLoopOnce's q->Recv (dist_loops_arch5.cc): take the next ticket and wait for its message
bool Engine::Receive(Batch *b) {
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t pos = __atomic_fetch_add(&queue_->dequeue_pos, 1, __ATOMIC_ACQ_REL);
  ggms_queue_header_t *h = QueueHeader(pos);
  const std::string what = "a batch from the samplers (ticket " + std::to_string(pos) + ")";
  if (!QueueWait(&h->seq, pos + 1, what.c_str(), true)) return false;
  b->queue_pos = pos;
  b->key = h->key;
  b->num_seeds = h->num_output;
  SAM_CHECK(b->num_seeds <= max_seeds_ && b->key < cfg.num_epoch * num_global_step_, "arch5: a queue slot with a bad header");
  b->recv_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return true;
}

// DoGraphCopy (dist_loops_arch5.cc): the slot's arrays into the batch's buffers on this GPU, one launch on xs; the
// slot goes back to the samplers as soon as that launch has completed (the timer's end: the host waits for it)
void Engine::Unpack(Batch *b, hipStream_t xs) {
  const ggms_queue_batch_t dst = b->trainer.View();
  SAM_GGMS(ggms_launch_timer_arm(b->handoff_timer));
  SAM_GGMS(ggms_queue_unpack(&dst, queue_slots_dev_ + (b->queue_pos % queue_depth_) * qlay_.slot_bytes, &qlay_, xs));
  double us = 0;
  SAM_GGMS(ggms_launch_timer_elapsed_us(b->handoff_timer, &us)); // blocks until the unpack has completed
  __atomic_store_n(&QueueHeader(b->queue_pos)->seq, b->queue_pos + queue_depth_, __ATOMIC_RELEASE); // free
}

} // namespace sam
