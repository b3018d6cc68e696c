// capi_dist.cpp — RCCL weight broadcast and streams on distinct hardware queues.
#include "capi_internal.hpp"

#include <dlfcn.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <fstream>
#include <thread>

using namespace mi::capi;

extern "C" {

// ------------------------------------------------------------------------------------------------ multi-GPU: weight broadcast
// The one exchange of the sharded path: the frozen .tflite bytes travel once from `root` to every rank over RCCL, then
// each rank builds its handles with mi_*_create_from_bytes.  A Rust host (north_star) has no torch.distributed: this entry speaks to
// librccl directly (loaded at call time, so the library itself does not depend on it).  Rendezvous = the ncclUniqueId in a file every
// rank of the node can read: `root` writes it (temporary name + rename), the others wait for it.
namespace {
struct UniqueId { char internal[128]; };   // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value like the original
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(UniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
}  // namespace

// ------------------------------------------------------------------------------------------------ streams on distinct hardware queues
// HIP streams share the device's hardware queues (GPU_MAX_HW_QUEUES, 4 by default) in the order they are first used; work on two streams of
// one queue runs strictly in order.  A host that keeps two batches in flight on two handles needs two streams that do NOT share a queue, and
// HIP has no call that tells: so the streams are created one by one and each candidate is TESTED — an idle wave of 40 us goes to every stream
// accepted so far and to the candidate at once; side by side the set takes 40 us, one after the other a multiple.
int mi_streams_create_distinct(int device, int n, void** streams) {
    return guarded([&] {
        require(streams != nullptr, "null argument");
        require(n >= 1 && n <= 4, "n must be 1 .. 4");
        mi::hip_check(hipSetDevice(device), "hipSetDevice");
        for (int k = 0; k < n; k++) streams[k] = nullptr;
        int* sink = nullptr;
        mi::hip_check(hipMalloc(reinterpret_cast<void**>(&sink), sizeof(int)), "hipMalloc");
        std::vector<hipStream_t> accepted, rejected;
        auto cleanup = [&](bool all) {
            for (hipStream_t s : rejected) hipStreamDestroy(s);
            if (all) for (hipStream_t s : accepted) hipStreamDestroy(s);
            hipFree(sink);
        };
        const long long ticks = 40 * 100;   // 40 us of the 100 MHz wall clock
        auto timed_together = [&](hipStream_t cand) {
            double best = 1e30;
            for (int rep = 0; rep < 3; rep++) {
                for (hipStream_t s : accepted) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
                mi::hip_check(hipStreamSynchronize(cand), "hipStreamSynchronize");
                const auto t0 = std::chrono::steady_clock::now();
                for (hipStream_t s : accepted)
                    if (mi::launch_spin(ticks, 1 << 20, sink, s) != 0) throw std::runtime_error("spin kernel launch failed");
                if (mi::launch_spin(ticks, 1 << 20, sink, cand) != 0) throw std::runtime_error("spin kernel launch failed");
                for (hipStream_t s : accepted) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
                mi::hip_check(hipStreamSynchronize(cand), "hipStreamSynchronize");
                best = std::min(best, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
            }
            return best;
        };
        try {
            for (int tries = 0; tries < 16 && static_cast<int>(accepted.size()) < n; tries++) {
                hipStream_t c = nullptr;
                mi::hip_check(hipStreamCreateWithFlags(&c, hipStreamNonBlocking), "hipStreamCreate");
                if (accepted.empty()) {
                    if (mi::launch_spin(ticks, 1 << 20, sink, c) != 0) throw std::runtime_error("spin kernel launch failed");   // (first use: the stream gets its queue)
                    mi::hip_check(hipStreamSynchronize(c), "hipStreamSynchronize");
                    accepted.push_back(c);
                    continue;
                }
                // side by side: about one idle wave (40 us + launch and synchronisation cost); sharing a queue with any accepted stream: two or more
                if (timed_together(c) < 1.6 * 40.0 + 30.0 * static_cast<double>(accepted.size())) accepted.push_back(c);
                else rejected.push_back(c);
            }
        } catch (...) {
            cleanup(true);
            throw;
        }
        if (static_cast<int>(accepted.size()) < n) {
            cleanup(true);
            throw ApiError(MI_EDEVICE, "could not find that many streams on distinct hardware queues (GPU_MAX_HW_QUEUES?)");
        }
        for (int k = 0; k < n; k++) streams[k] = accepted[static_cast<size_t>(k)];
        cleanup(false);
    });
}

int mi_streams_destroy(int device, int n, void** streams) {
    return guarded([&] {
        require(streams != nullptr && n >= 0, "bad argument");
        mi::hip_check(hipSetDevice(device), "hipSetDevice");
        for (int k = 0; k < n; k++)
            if (streams[k]) {
                mi::hip_check(hipStreamSynchronize(static_cast<hipStream_t>(streams[k])), "hipStreamSynchronize");
                mi::hip_check(hipStreamDestroy(static_cast<hipStream_t>(streams[k])), "hipStreamDestroy");
                streams[k] = nullptr;
            }
    });
}

int mi_dist_broadcast_bytes(const char* id_path, int rank, int world, int root, int device, uint8_t* buf, size_t nbytes, int timeout_ms) {
    return guarded([&] {
        require(id_path && buf, "null argument");
        require(world >= 1 && rank >= 0 && rank < world && root >= 0 && root < world, "rank / root outside [0, world)");
        require(nbytes > 0 && nbytes <= (static_cast<size_t>(1) << 31), "nbytes must be in (0, 2 GiB]");
        mi::hip_check(hipSetDevice(device), "hipSetDevice");
        static std::mutex mu;
        static Rccl R;
        {
            std::lock_guard<std::mutex> g(mu);
            if (!R.lib) {
                void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
                if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
                if (!lib) throw ApiError(MI_EDEVICE, std::string("librccl is not loadable: ") + dlerror());
                auto sym = [&](const char* n) {
                    void* p = dlsym(lib, n);
                    if (!p) throw ApiError(MI_EDEVICE, std::string("librccl lacks ") + n);
                    return p;
                };
                R.GetUniqueId = reinterpret_cast<decltype(R.GetUniqueId)>(sym("ncclGetUniqueId"));
                R.CommInitRank = reinterpret_cast<decltype(R.CommInitRank)>(sym("ncclCommInitRank"));
                R.Broadcast = reinterpret_cast<decltype(R.Broadcast)>(sym("ncclBroadcast"));
                R.CommDestroy = reinterpret_cast<decltype(R.CommDestroy)>(sym("ncclCommDestroy"));
                R.GetErrorString = reinterpret_cast<decltype(R.GetErrorString)>(sym("ncclGetErrorString"));
                R.lib = lib;
            }
        }
        auto nccl = [&](int rc, const char* what) {
            if (rc != 0) throw ApiError(MI_EDEVICE, std::string(what) + ": " + (R.GetErrorString ? R.GetErrorString(rc) : "rccl error"));
        };
        UniqueId id{};
        const std::string path = id_path, tmp = path + ".tmp";
        // rendezvous file: {"MIRV", world, root} + the 128-byte id.  A file of another job shape is never taken for this one's; a stale file of the
        // SAME shape (a crashed earlier run under a reused name) cannot be told from a root that was simply early — for that case ncclCommInitRank
        // runs under the caller's timeout below instead of blocking for ever.
        const uint32_t head[3] = {0x5652494du, static_cast<uint32_t>(world), static_cast<uint32_t>(root)};
        if (rank == root) {
            std::remove(path.c_str());   // whatever an earlier run left under this name
            nccl(R.GetUniqueId(&id), "ncclGetUniqueId");
            {
                std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
                if (!f || !f.write(reinterpret_cast<const char*>(head), sizeof head) || !f.write(id.internal, sizeof id.internal))
                    throw ApiError(MI_EIO, "cannot write the rendezvous file '" + tmp + "'");
            }
            if (std::rename(tmp.c_str(), path.c_str()) != 0) throw ApiError(MI_EIO, "cannot publish the rendezvous file '" + path + "'");
        } else {
            const auto t0 = std::chrono::steady_clock::now();
            for (;;) {
                std::ifstream f(path, std::ios::binary);
                uint32_t got[3] = {0, 0, 0};
                if (f && f.read(reinterpret_cast<char*>(got), sizeof got) && got[0] == head[0] && got[1] == head[1] && got[2] == head[2] &&
                    f.read(id.internal, sizeof id.internal) && f.gcount() == static_cast<std::streamsize>(sizeof id.internal))
                    break;
                if (timeout_ms >= 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms))
                    throw ApiError(MI_EIO, "no rendezvous file '" + path + "' of this job (world " + std::to_string(world) + ", root " + std::to_string(root) + ") from the root rank within the timeout");
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
            }
        }
        void* comm = nullptr;
        uint8_t* d = nullptr;
        hipStream_t s = nullptr;
        try {
            if (timeout_ms >= 0 && world > 1) {
                // bounded: a communicator that does not form (a stale id, a rank that died) must not hang the caller.  The call cannot be cancelled; on
                // a timeout its thread is left behind and the caller gets MI_EIO (and is expected to exit)
                struct Init { std::mutex m; std::condition_variable cv; bool done = false; int rc = 0; void* comm = nullptr; };
                auto st = std::make_shared<Init>();
                auto fn = R.CommInitRank;
                std::thread([st, fn, world, id, rank, device] {
                    hipSetDevice(device);
                    void* c = nullptr;
                    const int rc = fn(&c, world, id, rank);
                    std::lock_guard<std::mutex> g(st->m);
                    st->rc = rc; st->comm = c; st->done = true;
                    st->cv.notify_all();
                }).detach();
                std::unique_lock<std::mutex> lk(st->m);
                // (the id exchange itself is quick; the bound is the caller's timeout, at least 10 s for the bootstrap of a whole node)
                if (!st->cv.wait_for(lk, std::chrono::milliseconds(std::max(timeout_ms, 10000)), [&] { return st->done; }))
                    throw ApiError(MI_EIO, "ncclCommInitRank did not complete within the timeout (a stale rendezvous file '" + path + "', or a rank that never arrived)");
                comm = st->comm;
                nccl(st->rc, "ncclCommInitRank");
            } else {
                nccl(R.CommInitRank(&comm, world, id, rank), "ncclCommInitRank");
            }
            if (rank == root) std::remove(path.c_str());   // every rank has read it: CommInitRank is collective
            mi::hip_check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
            mi::hip_check(hipMalloc(reinterpret_cast<void**>(&d), nbytes), "hipMalloc");
            if (rank == root) mi::hip_check(hipMemcpyAsync(d, buf, nbytes, hipMemcpyHostToDevice, s), "H2D model bytes");
            nccl(R.Broadcast(d, d, nbytes, /* ncclUint8 */ 1, root, comm, s), "ncclBroadcast");
            if (rank != root) mi::hip_check(hipMemcpyAsync(buf, d, nbytes, hipMemcpyDeviceToHost, s), "D2H model bytes");
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        } catch (...) {
            if (d) hipFree(d);
            if (s) hipStreamDestroy(s);
            if (comm) R.CommDestroy(comm);
            throw;
        }
        hipFree(d);
        hipStreamDestroy(s);
        nccl(R.CommDestroy(comm), "ncclCommDestroy");
    });
}

}  // extern "C"
