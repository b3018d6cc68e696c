// engine.cpp — see engine.hpp.
#include "engine.hpp"
#include "launch.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace mi {

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

namespace {
template <class T>  // dev becomes a device copy of host (none when host is empty); the host copy is not needed again and is freed
void upload(T*& dev, std::vector<T>& host, const char* what_alloc, const char* what_copy) {
    if (dev) hip_check(hipFree(dev), "hipFree");
    dev = nullptr;
    if (host.empty()) return;
    hip_check(hipMalloc(reinterpret_cast<void**>(&dev), host.size() * sizeof(T)), what_alloc);
    hip_check(hipMemcpy(dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice), what_copy);
    std::vector<T>().swap(host);
}
}  // namespace

Model::Model(const uint8_t* bytes, size_t n, int device) : device_(device), blob_(bytes, bytes + n) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        throw std::runtime_error("no HIP device visible: the MI355X kernels cannot run (no CPU fallback exists)");
    if (device < 0 || device >= count) throw std::runtime_error("device ordinal out of range");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hipDeviceProp_t prop;
    hip_check(hipGetDeviceProperties(&prop, device_), "hipGetDeviceProperties");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        throw std::runtime_error(std::string("kernels are built for gfx950 only; device is ") + prop.gcnArchName);
    hip_check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    rebuild();
}

Model::~Model() {
    hipSetDevice(device_);
    invalidate_graphs();
    if (d_weights_) hipFree(d_weights_);
    if (d_programs_) hipFree(d_programs_);
    if (d_tail_programs_) hipFree(d_tail_programs_);
    if (d_arena_) hipFree(d_arena_);
    if (d_small_) hipFree(d_small_);
    if (d_in_stage_) hipFree(d_in_stage_);
    free_bandnet();
    for (float* p : d_out_)
        if (p) hipFree(p);
    for (hipStream_t st : side_streams_) hipStreamDestroy(st);
    for (hipEvent_t ev : lane_events_) hipEventDestroy(ev);
    for (hipStream_t st : head_streams_) hipStreamDestroy(st);
    for (hipEvent_t ev : head_events_) if (ev) hipEventDestroy(ev);
    if (stream_) hipStreamDestroy(stream_);
}

void Model::invalidate_graphs() {
    // a replay may still be running on a caller's stream (asynchronous entry points): let the device drain first
    if (!graphs_.empty()) (void)hipDeviceSynchronize();
    for (auto& kv : graphs_) hipGraphExecDestroy(kv.second);
    graphs_.clear();
}

// The options: one row per key.  A set clamps the value into [lo, hi] (a [0, 1] range is a switch: every value but 0 is stored as 1), then invalidates
// the captured graphs and has the arena laid out again on the next run; `flags` says what else it does, or what the key does differently.
struct Model::Option {
    enum { kReplan = 1,      // the plan depends on it: lowered and packed again before the next run (dirty_)
           kFreeSmall = 2,   // the small-batch scratch is sized by it
           kKeepGraphs = 4,  // touches neither graphs nor arena
           kOneOf = 8,       // lo is a set instead: bit v says that v is accepted, every other value is stored as 0
           kKiB = 16 /* set and read in KiB, stored in bytes */, kWriteOnly = 32, kReadOnly = 64,
           kBandGen = 128,   // stored in band_gen_, and the next band launch takes the wrap path (band_gen_force_)
           kForms = 256 };   // a switch that grew further positions: lo .. hi are accepted, every other value is stored as 1
    const char* key;
    int Model::*field;
    int lo, hi, flags;
};

const Model::Option* Model::find_option(const std::string& key) {
    using O = Option;
    constexpr int kMax = 0x7fffffff;
    static const Option table[] = {
        {"chunk", &Model::chunk_, 0, kMax, 0},  // frames per chunk of a run (0: chosen per run)
        {"graph", &Model::use_graph_, 0, 1, 0},  // 0: eager launches instead of hipGraph replay
        {"fuse", &Model::fuse_level_, 0, 5, O::kReplan},  // fusion level of the lowering (plan.hpp)
        {"res_budget", &Model::res_budget_, 16, 156, O::kReplan | O::kKiB},  // LDS (KiB) a stage program may use
        {"pipe", &Model::pipe_max_, 0, 4, O::kReplan},  // blocks per row-pipelined chain (level 4)
        {"small_chain", &Model::small_chain_, 0, 64, O::kFreeSmall},  // frames up to which a row-pipelined chain runs one launch per block (0: never)
        // row pipeline: 1 = one row per step (strip_pipe_kernel), 2 = two rows, packed-FMA pointwise convs (strip_pipe2_kernel), 4 = one row, MFMA pointwise convs (strip_pipe1m_kernel)
        {"pipe_rows", &Model::pipe_rows_, 1 << 1 | 1 << 2 | 1 << 4, 0, O::kOneOf},
        {"pipe_band", &Model::pipe_band_, 0, 4096, 0},  // rows per band of the row pipelines (0: automatic)
        {"strip", &Model::strip_, 0, 1, 0},  // 0: none of the strip / operand-layout kernels runs (blocks stay on the block kernel and its fused forms)
        {"stem_fuse", &Model::stem_fuse_, 0, 1, 0},  // 0: the first convolution keeps its own launch in front of the face mesh's block pair (mdblock_kernel<stem+pair>)
        // the detectors' 5x5 first convolution (bit-identical in all three): 1 = stem_mfma_kernel, the window's picture rows kept in registers down a column of tiles;
        // 2 = the row-wise MFMA form (every tile loads its five rows); 0 = stem_conv_kernel (packed VALU FMAs) at every batch size
        {"stem_mfma", &Model::stem_mfma_, 0, 2, O::kForms},
        {"conv_mfma", &Model::conv_mfma_, 0, 1, 0},  // 0: the dense k x k convolutions with C % 32 == 0 stay on conv_generic_kernel instead of conv_mfma_kernel (the matrix cores)
        // the same convolutions (whatever "conv_mfma" says) on the bf16 matrix cores, conv_bf16_kernel: 1 = activations and filter values rounded to bf16 (nearest even),
        // products accumulated in f32; 2 = every operand split into two bf16 values, three products for one (about f32 accuracy); 0 = as without the option, bit for bit
        {"conv_bf16", &Model::conv_bf16_, 0, 2, O::kReplan},
        {"stem_run", &Model::stem_run_, 0, 32, 0},  // output rows per column run of stem_mfma_kernel (0: chosen per launch, the row-wise form where a run would be one row)
        {"pair_fuse", &Model::pair_fuse_, 0, 1, 0},  // 0: two plain blocks in a row keep a launch each (the face mesh's 48x48x32 blocks: mwalk_kernel), no mdblock_kernel<pair>
        {"mdb_band", &Model::mdb_band_, 0, 4096, 0},  // rows per band of the mdblock_kernel launches (0: chosen per launch)
        {"chain_fixed", &Model::chain_fixed_, 0, 1, 0},  // 0: the frame-resident chain launches always take the generic kernel (bit-identical), never a fixed-shape instantiation
        {"chain_sched", &Model::chain_sched_, 0, 1, 0},  // fixed-shape chain launches: 1 = contraction in phases (LDS reads a chunk ahead, FMAs as a block, MFMAs as a block), 0 = MFMAs interleaved with the next chunk's taps (bit-identical)
        {"mchain", &Model::mchain_, 0, 1, 0},  // 0: the 32x32x48 blocks run one launch each (mstrip_kernel) instead of one launch per run
        {"tail", &Model::tail_, 0, 1, O::kReplan},  // 0: no stage program runs on tail_kernels.hip
        {"tail_pre", &Model::tail_pre_, 0, 2, 0},  // tail programs: 0 = chosen per launch, 1 = constants a stage ahead (one workgroup per CU), 2 = 128 registers (two per CU)
        {"tail_g", &Model::tail_g_, 0, 64, 0},  // frames per workgroup of the tail stage programs (0: chosen per launch)
        {"band", &Model::band_, 0, 2, O::kReplan},  // single-launch plan: 0 never, 1 one_shot runs (the single-image entries), 2 every run of few enough frames
        {"band_test_fail", &Model::band_test_fail_, 0, 1, O::kWriteOnly},  // test hook: the next single-launch run reports that it gave up
        {"band_test_absent", &Model::band_test_absent_, 0, 256, O::kWriteOnly},  // test hook: every k-th workgroup of a single-launch run leaves at once without publishing (0: off)
        {"band_test_gen", nullptr, 0, kMax, O::kBandGen | O::kWriteOnly},  // test hook: the host's count of band launches (the packet tags wrap at 2^26: see run_device)
        {"band_wide", &Model::band_wide_ok_, 0, 1, O::kReplan},  // single-launch plan: stages of more than 128 channels (0: the program ends in front of the first one)
        {"band_fork", &Model::band_fork_, 0, 1, O::kReplan},  // single-launch plan: the second branch behind a fork on the idle workgroups
        {"band_nw", &Model::band_nw_, 8, 256, O::kReplan},  // single-launch plan: most workgroups per frame
        {"band_fail_streak", &Model::band_fail_streak_, 0, 0, O::kReadOnly},  // single launches in a row that gave up
        {"band_wraps", &Model::band_wraps_, 0, 0, O::kReadOnly},  // times the band workspace was cleared because the packet tags wrapped
        {"fork", &Model::fork_, 0, 1, 0},  // 0: output heads and tail branches stay on the trunk's stream
        {"heads", &Model::head_streams_opt_, 1, kHeadStreams, O::kReplan},  // side streams the output heads are spread over
        {"reuse", &Model::reuse_, 0, 1, O::kReplan},  // 0: debugging layout, every tensor keeps its own arena slot
        {"lanes", &Model::lanes_, 1, 4, 0},  // chunks of a run in flight on streams of their own
        {"test_poison", &Model::test_poison_, 1 << 1 | 1 << 2, 0, O::kOneOf | O::kKeepGraphs},  // test hook: fill the scratch and output buffers before every run (poison_scratch)
    };
    for (const Option& o : table)
        if (key == o.key) return &o;
    return nullptr;
}

void Model::set_option(const std::string& key, int value) {
    const Option* o = find_option(key);
    if (!o || (o->flags & Option::kReadOnly)) throw std::runtime_error("unknown option '" + key + "'");
    int v = (o->lo == 0 && o->hi == 1) ? value != 0 : std::min(o->hi, std::max(o->lo, value));
    if (o->flags & Option::kOneOf) v = (value >= 0 && value < 31 && (o->lo >> value & 1)) ? value : 0;
    if (o->flags & Option::kForms) v = (value >= o->lo && value <= o->hi) ? value : 1;
    if (o->flags & Option::kKiB) v *= 1024;
    if (o->flags & Option::kBandGen) { band_gen_ = static_cast<unsigned>(v); band_gen_force_ = true; }
    else this->*o->field = v;
    if (o->flags & Option::kKeepGraphs) return;
    if (o->flags & Option::kReplan) dirty_ = true;
    if ((o->flags & Option::kFreeSmall) && d_small_) { hipFree(d_small_); d_small_ = nullptr; small_floats_ = 0; }
    invalidate_graphs();
    chunk_cap_ = 0;  // arena is re-laid out on the next run
}

int Model::get_option(const std::string& key) const {
    const Option* o = find_option(key);
    if (!o || (o->flags & Option::kWriteOnly)) throw std::runtime_error("unknown option '" + key + "'");
    const int v = this->*o->field;
    return (o->flags & Option::kKiB) ? v / 1024 : v;
}

void Model::rebuild() {
    if (d_small_) { hipFree(d_small_); d_small_ = nullptr; small_floats_ = 0; }  // sized for the plan it was allocated under
    hip_check(hipSetDevice(device_), "hipSetDevice");
    invalidate_graphs();
    plan_ = build_plan(parse_tflite(blob_.data(), blob_.size()), fuse_level_, pipe_max_, res_budget_, tail_ != 0);
    if (!reuse_) {  // debugging layout: every tensor keeps its own slot
        long off = 0;
        for (size_t t = 0; t < plan_.graph.tensors.size(); t++)
            if (plan_.root_offset[t] >= 0) { plan_.root_offset[t] = off; off += plan_.root_elems[t]; }
        plan_.arena_floats_per_frame = off;
    }
    consts_ = pack_plan_consts(plan_, conv_bf16_);  // every constant the launches need and the stage programs (consts.cpp)
    upload(d_weights_, consts_.blob, "hipMalloc weights", "upload weights");  // (never empty: the blob ends in its slack)
    upload(d_tail_programs_, consts_.tail_progs, "hipMalloc programs", "upload programs");
    upload(d_programs_, consts_.progs, "hipMalloc programs", "upload programs");
    sched_ = schedule_side_streams(plan_, head_streams_opt_);  // which nodes run beside the trunk (launches.cpp)
    build_bandnet();
    dirty_ = false;
    chunk_cap_ = 0;
}

void Model::free_bandnet() {
    if (d_band_prog_) hipFree(d_band_prog_);
    if (d_band_consts_) hipFree(d_band_consts_);
    if (d_band_ws_) hipFree(d_band_ws_);
    if (d_band_sync_) hipFree(d_band_sync_);
    if (h_band_fail_) hipHostFree(h_band_fail_);
    d_band_prog_ = nullptr; d_band_consts_ = nullptr; d_band_ws_ = nullptr; d_band_sync_ = nullptr; h_band_fail_ = nullptr; d_band_fail_ = nullptr;
    band_plan_ = BandPlan();
}

// The single-launch plan (bandnet_kernels.hip) of the same graph: planned on the host from the level-2 lowering (build_band_plan, bandplan.cpp);
// here it is uploaded and given its workspace, its sync words and its fail word.  A graph without such a plan leaves the handle on the batched plan
void Model::build_bandnet() {
    free_bandnet();
    if (!band_ || fuse_level_ < 2) return;
    BandOptions o;
    o.nw = band_nw_; o.wide = band_wide_ok_ != 0; o.fork = band_fork_ != 0; o.cu_count = device_cu_count();
    band_plan_ = build_band_plan(plan_, build_plan(parse_tflite(blob_.data(), blob_.size()), 2), o);
    upload(d_band_prog_, band_plan_.prog, "hipMalloc band program", "upload band program");
    upload(d_band_consts_, band_plan_.consts, "hipMalloc band constants", "upload band constants");
    if (!band_plan_.ready) return;
    band_ws_bytes_ = static_cast<size_t>(band_plan_.ws_frame_floats) * band_plan_.max_frames * sizeof(float);
    hip_check(hipMalloc(reinterpret_cast<void**>(&d_band_ws_), band_ws_bytes_), "hipMalloc band workspace");
    hip_check(hipMemset(d_band_ws_, 0, band_ws_bytes_), "hipMemset");   // no packet carries a tag yet (tags start at 1)
    hip_check(hipMalloc(reinterpret_cast<void**>(&d_band_sync_), 64 * sizeof(unsigned)), "hipMalloc band generation");
    hip_check(hipMemset(d_band_sync_, 0, 64 * sizeof(unsigned)), "hipMemset");
    hip_check(hipHostMalloc(reinterpret_cast<void**>(&h_band_fail_), 64, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
    *h_band_fail_ = 0;
    hip_check(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_band_fail_), h_band_fail_, 0), "hipHostGetDevicePointer");
}

void Model::ensure_capacity(int batch) {
    int chunk = chunk_ > 0 ? std::min(chunk_, batch) : batch;
    if (lanes_ > 1) chunk = std::min(chunk, (batch + lanes_ - 1) / lanes_);  // each lane owns one arena region
    if (chunk > chunk_cap_ || static_cast<size_t>(plan_.arena_floats_per_frame) * chunk * lanes_ > arena_floats_) {
        invalidate_graphs();
        if (d_arena_) hip_check(hipFree(d_arena_), "hipFree arena");
        d_arena_ = nullptr;
        chunk = std::max(chunk, chunk_cap_);
        arena_floats_ = static_cast<size_t>(plan_.arena_floats_per_frame) * chunk * lanes_;
        hip_check(hipMalloc(reinterpret_cast<void**>(&d_arena_), std::max<size_t>(arena_floats_, 64) * sizeof(float)), "hipMalloc arena");
        chunk_cap_ = chunk;
    }
    if (!d_small_ && small_chain_ > 0) {  // ping-pong scratch of the small-batch form of the row-pipelined chains (fixed size: replay graphs hold the pointer)
        size_t fmax = 0;
        for (const Node& n : plan_.nodes)
            if (n.kind == Node::Chain) {
                const auto& sh = plan_.graph.tensors[n.in[0]].shape;
                if (sh.size() == 4 && sh[1] * sh[2] > 256) fmax = std::max(fmax, static_cast<size_t>(sh[1]) * sh[2] * sh[3]);
            }
        if (fmax) {
            small_floats_ = 2 * static_cast<size_t>(small_chain_) * fmax;
            hip_check(hipMalloc(reinterpret_cast<void**>(&d_small_), small_floats_ * sizeof(float)), "hipMalloc small-batch scratch");
        }
    }
    if (batch > batch_cap_) {
        invalidate_graphs();
        for (float* p : d_out_)
            if (p) hip_check(hipFree(p), "hipFree out");
        d_out_.assign(num_outputs(), nullptr);
        for (int k = 0; k < num_outputs(); k++)
            hip_check(hipMalloc(reinterpret_cast<void**>(&d_out_[k]), output_elems(k) * sizeof(float) * batch), "hipMalloc outputs");
        batch_cap_ = batch;
    }
}

std::vector<Model::LaunchStat> Model::profile(const float* in, int batch, int reps, hipStream_t stream) {
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (dirty_) rebuild();
    ensure_capacity(batch);
    hipStream_t s = stream ? stream : stream_;
    const Graph& g = plan_.graph;
    // one untimed pass first: the first launch of a kernel symbol in a process loads its code object (about a millisecond,
    // which averaged over a few reps made the first layer of every kernel type look 3x slower than its twins)
    profile_inner_ = 4;
    band_use_ = band_ == 2 && band_usable(batch);
    std::vector<hipEvent_t> marks;
    Lowered first;             // the first chunk's launches: one record each (a shorter last chunk may take other kernels: its time goes by plan node)
    std::vector<double> ms;
    for (int r = -1; r < reps; r++) {
        marks.clear();
        std::vector<Lowered> chunks;
        for (int start = 0; start < batch; start += chunk_cap_) {
            chunks.emplace_back();
            enqueue_chunk(in, start, std::min(chunk_cap_, batch - start), s, &marks, &chunks.back());
        }
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (r < 0) { first = chunks[0]; ms.assign(first.launches.size(), 0.0); }
        size_t m = 0;
        for (const Lowered& c : chunks) {
            if (m + c.launches.size() + 1 > marks.size()) throw std::runtime_error("internal: profile marks mismatch");
            for (const Launch& l : c.launches) {
                float t = 0;
                hip_check(hipEventElapsedTime(&t, marks[m], marks[m + 1]), "hipEventElapsedTime");
                if (r >= 0) ms[static_cast<size_t>(first.launch_of_node[static_cast<size_t>(l.node)])] += t / reps / profile_inner_;
                m++;
            }
            m++;
        }
        if (m != marks.size()) throw std::runtime_error("internal: profile marks mismatch");
        for (hipEvent_t ev : marks) hipEventDestroy(ev);
    }
    profile_inner_ = 1;
    band_use_ = false;
    // a plan node's bytes and MACs belong to the launch that stands for it
    std::vector<LaunchStat> stats(first.launches.size());
    for (size_t k = 0; k < stats.size(); k++) { stats[k].kernel = first.launches[k].label; stats[k].ms = ms[k]; }
    for (size_t i = 0; i < plan_.nodes.size(); i++) {
        const Node& n = plan_.nodes[i];
        if (first.launch_of_node[i] < 0) continue;
        const size_t k = static_cast<size_t>(first.launch_of_node[i]);
        LaunchStat& st = stats[k];
        auto elems = [&](int t) { return t >= 0 ? static_cast<double>(g.tensors[t].elems()) : 0.0; };
        double per_frame = 4 * elems(n.out);
        for (int t : n.in) per_frame += 4 * elems(t);
        if (n.res >= 0 && !(n.kind == Node::Block && n.res == n.in[0])) per_frame += 4 * elems(n.res);
        double weights = 0, macs = 0;
        for (int c : {n.w, n.b, n.w2, n.b2, n.alpha}) weights += 4 * elems(c);
        double bytes = per_frame * batch + weights;
        const auto& si = g.tensors[n.in[0]].shape;
        const auto& so = g.tensors[n.out].shape;
        if (n.kind == Node::Conv) macs = elems(n.out) * n.KH * n.KW * si.back() * batch;
        if (n.kind == Node::Dw) macs = elems(n.out) * n.KH * n.KW * batch;
        if (n.kind == Node::Block) macs = elems(n.out) / so.back() * si.back() * ((n.w >= 0 ? 9 : 0) + so.back()) * batch;
        if (n.kind == Node::Resident) {
            for (int t : n.extra_out) bytes += 4 * elems(t) * batch;
            for (const Node& m : n.members) {
                const auto& mo = g.tensors[m.out].shape;
                const int Cm = g.tensors[m.in[0]].shape[3];
                if (m.kind == Node::Conv) macs += elems(m.out) * m.KH * m.KW * Cm * batch;
                else macs += static_cast<double>(mo[1]) * mo[2] * Cm * ((m.w >= 0 ? 9 : 0) + mo[3]) * batch;
                for (int c : {m.w, m.b, m.w2, m.b2, m.alpha}) bytes += 4 * elems(c);
            }
        }
        if (n.kind == Node::Chain) {
            for (int t : n.extra_out) bytes += 4 * elems(t) * batch;
            for (const Node& m : n.members) {
                const auto& mo = g.tensors[m.out].shape;
                macs += static_cast<double>(mo[1]) * mo[2] * g.tensors[m.in[0]].shape[3] * (9 + mo[3]) * batch;
            }
            for (const Node& m : n.members)
                for (int c : {m.w, m.b, m.w2, m.b2, m.alpha}) bytes += 4 * elems(c);
            for (const Node& m : n.head_nodes) {
                macs += elems(m.out) * g.tensors[m.in[0]].shape[3] * batch;
                for (int c : {m.w, m.b, m.w2, m.b2}) bytes += 4 * elems(c);
            }
        }
        st.bytes += bytes;
        st.macs += macs;
        // input shape of the launch's first node -> output shape of its last
        auto dims = [](const std::vector<int>& sh) {
            std::string d;
            for (size_t q = 1; q < sh.size(); q++) d += (q > 1 ? "x" : "") + std::to_string(sh[q]);
            return d;
        };
        if (static_cast<int>(i) == first.launches[k].node) st.detail = dims(si) + "->";
        st.detail = st.detail.substr(0, st.detail.find("->") + 2) + dims(so);
    }
    return stats;
}

LaunchCtx Model::launch_ctx(const float* in, int chunk_start, int frames) const {
    LaunchCtx c;
    c.weights = d_weights_;
    c.arena = d_arena_ + static_cast<size_t>(plan_.arena_floats_per_frame) * chunk_cap_ * arena_lane_;
    c.in = in; c.out = d_out_.data();
    c.small = d_small_; c.small_floats = small_floats_;
    c.progs = d_programs_; c.tail_progs = d_tail_programs_;
    c.band_prog = d_band_prog_; c.band_consts = d_band_consts_; c.band_ws = d_band_ws_; c.band_sync = d_band_sync_; c.band_fail = d_band_fail_;
    c.chunk_cap = chunk_cap_; c.chunk_start = chunk_start; c.F = frames;
    c.u8_frames = u8_.frames; c.u8_lut = u8_.lut; c.u8_frame_bytes = u8_.frame_bytes; c.u8_row_bytes = u8_.row_bytes;
    c.strip = strip_; c.pair_fuse = pair_fuse_; c.stem_fuse = stem_fuse_; c.stem_mfma = stem_mfma_; c.stem_run = stem_run_; c.mchain = mchain_; c.conv_mfma = conv_mfma_; c.conv_bf16 = conv_bf16_;
    c.small_chain = small_chain_; c.lanes = lanes_;
    c.pipe_rows = pipe_rows_; c.pipe_band = pipe_band_; c.mdb_band = mdb_band_; c.tail_pre = tail_pre_; c.tail_g = tail_g_;
    // (with several lanes the chunks already overlap; the head streams and node events are one set per model, and sharing
    // them between concurrently recorded lanes crashes the graph)
    c.fork = fork_ && lanes_ == 1;
    c.cu_count = device_cu_count();
    c.band = band_use_ && chunk_start == 0;
    c.band_test_absent = band_test_absent_;
    return c;
}

namespace {
int issue(const Launch& l, hipStream_t s, int chain_fixed, int chain_sched) {
    auto many = [&](int (*f)(const BlockArgs*, int, void*)) { return f(l.blocks.data(), static_cast<int>(l.blocks.size()), s); };
    switch (l.to) {
        case Launcher::Conv: return launch_conv(std::get<ConvArgs>(l.args), s);
        case Launcher::HeadGemm: return launch_head_gemm(std::get<HeadGemmArgs>(l.args), s);
        case Launcher::Dw: return launch_dw(std::get<DwArgs>(l.args), s);
        case Launcher::Xc: return launch_xc(std::get<XcArgs>(l.args), s);
        case Launcher::Mdblock: return launch_mdblock(std::get<DblockArgs>(l.args), s);
        case Launcher::Dblock: return launch_dblock(std::get<DblockArgs>(l.args), s);
        case Launcher::Mbneck: return launch_mbneck(std::get<BneckArgs>(l.args), s);
        case Launcher::Bneck: return launch_bneck(std::get<BneckArgs>(l.args), s);
        case Launcher::Tail: return launch_tail(std::get<TailLaunch>(l.args), s);
        case Launcher::Resident: return launch_resident(std::get<ResLaunch>(l.args), s);
        case Launcher::Chain: return launch_chain(std::get<ChainArgs>(l.args), s, chain_fixed, chain_sched);
        case Launcher::StripPipe: return many(launch_strip_pipe);
        case Launcher::MstripChain: return many(launch_mstrip_chain);
        case Launcher::SmallChain: {
            int rc = 0;
            for (size_t k = 0; k < l.blocks.size() && rc == 0; k++) rc = l.blocks[k].sh == 1 ? launch_strip(l.blocks[k], s) : launch_block(l.blocks[k], s);
            return rc;
        }
        case Launcher::Ms2: return launch_ms2(std::get<BlockArgs>(l.args), s);
        case Launcher::Mwalk: return launch_mwalk(std::get<BlockArgs>(l.args), s);
        case Launcher::Strip: return launch_strip(std::get<BlockArgs>(l.args), s);
        case Launcher::Mstrip: return launch_mstrip(std::get<BlockArgs>(l.args), s);
        case Launcher::Block: return launch_block(std::get<BlockArgs>(l.args), s);
        case Launcher::Add: return launch_add(std::get<EltArgs>(l.args), s);
        case Launcher::Act: return launch_act(std::get<EltArgs>(l.args), s);
        case Launcher::Maxpool: return launch_maxpool(std::get<EltArgs>(l.args), s);
        case Launcher::Padc: return launch_padc(std::get<EltArgs>(l.args), s);
        case Launcher::Resize2x: return launch_resize2x(std::get<EltArgs>(l.args), s);
        case Launcher::DepthToSpace: return launch_depth_to_space(std::get<EltArgs>(l.args), s);
        case Launcher::Bandnet: return launch_bandnet(std::get<BandLaunch>(l.args), s);
        case Launcher::Avgpool: return launch_avgpool(std::get<EltArgs>(l.args), s);
        case Launcher::L2norm: return launch_l2norm_rows(std::get<EltArgs>(l.args), s);
        case Launcher::Transpose: return launch_transpose(std::get<EltArgs>(l.args), s);
    }
    return 0;
}
}  // namespace

// Issues one chunk: the launch list comes from lower_chunk (launches.cpp); here are the streams, the events and the profiling marks.
// keep: the list that was issued, with its labels (profile())
void Model::enqueue_chunk(const float* in, int chunk_start, int F, hipStream_t trunk, std::vector<hipEvent_t>* marks, Lowered* keep) {
    LaunchCtx ctx = launch_ctx(in, chunk_start, F);
    if (marks) ctx.fork = false;  // (the per-launch events of profiling assume one stream)
    Lowered low = lower_chunk(plan_, consts_, band_plan_, sched_, ctx, keep != nullptr);
    auto mark = [&] {
        if (!marks) return;
        hipEvent_t ev;
        hip_check(hipEventCreate(&ev), "hipEventCreate");
        hip_check(hipEventRecord(ev, trunk), "hipEventRecord");  // profiling marks: eager launches only
        marks->push_back(ev);
    };
    mark();
    // events: one per launch (by its index), one for the start of the plan, one per side stream for the join
    const size_t n_launches = low.launches.size(), start_event = plan_.nodes.size();
    auto event = [&](size_t k) {
        if (head_events_.size() < plan_.nodes.size() + 2 + kHeadStreams) head_events_.resize(plan_.nodes.size() + 2 + kHeadStreams, nullptr);
        if (!head_events_[k]) hip_check(hipEventCreateWithFlags(&head_events_[k], hipEventDisableTiming), "hipEventCreate");
        return head_events_[k];
    };
    unsigned used_heads = 0;
    for (size_t k = 0; k < n_launches; k++) {
        const Launch& l = low.launches[k];
        hipStream_t s = trunk;
        if (l.slot >= 0) {
            while (static_cast<int>(head_streams_.size()) <= l.slot) {
                hipStream_t st;
                hip_check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
                head_streams_.push_back(st);
            }
            s = head_streams_[static_cast<size_t>(l.slot)];
            if (l.wait >= 0) {
                hip_check(wait_event(s, event(static_cast<size_t>(low.launch_of_node[static_cast<size_t>(l.wait)]))), "hipStreamWaitEvent");
            } else {  // reads the graph input: order it behind whatever the trunk stream was doing before this plan
                hip_check(record_event(event(start_event), trunk), "hipEventRecord");
                hip_check(wait_event(s, event(start_event)), "hipStreamWaitEvent");
            }
            used_heads |= 1u << l.slot;
        }
        // profiling: the launch is repeated between its two marks (a launch never reads what it writes), so that the event bubble
        // between marks is shared by profile_inner_ executions and the per-launch figure approaches rocprofv3's kernel duration
        int rc = 0;
        for (int rep = 0; rep < (marks ? profile_inner_ : 1) && rc == 0; rep++) rc = issue(l, s, chain_fixed_, chain_sched_);
        if (rc != 0) throw std::runtime_error(std::string("kernel launch failed: ") + hipGetErrorString(static_cast<hipError_t>(rc)));
        if (l.record) hip_check(record_event(event(k), s), "hipEventRecord");
        mark();
    }
    for (int k = 0; k < kHeadStreams; k++)  // join: the trunk stream continues (post-processing, the next chunk) after every head
        if (used_heads & (1u << k)) {
            hip_check(record_event(event(start_event + 1 + static_cast<size_t>(k)), head_streams_[static_cast<size_t>(k)]), "hipEventRecord");
            hip_check(wait_event(trunk, event(start_event + 1 + static_cast<size_t>(k))), "hipStreamWaitEvent");
        }
    last_chunk_frames_ = F;
    if (keep) *keep = std::move(low);
}

void Model::enqueue_all(const float* in, int batch, hipStream_t s) {
    if (lanes_ > 1 && batch > chunk_cap_) {
        // Independent frame ranges on concurrent streams: while one lane is in its small, latency-bound tail layers the
        // other lanes' large layers keep the CUs busy.  Fork/join with events (captured as parallel graph branches).
        while (static_cast<int>(side_streams_.size()) < lanes_ - 1) {
            hipStream_t st;
            hip_check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
            side_streams_.push_back(st);
        }
        while (static_cast<int>(lane_events_.size()) < lanes_) {
            hipEvent_t ev;
            hip_check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
            lane_events_.push_back(ev);
        }
        hip_check(record_event(lane_events_[0], s), "hipEventRecord");
        int lane = 0;
        for (int start = 0; start < batch; start += chunk_cap_, lane = (lane + 1) % lanes_) {
            hipStream_t ls = lane == 0 ? s : side_streams_[lane - 1];
            if (lane > 0 && start < chunk_cap_ * lanes_) hip_check(wait_event(ls, lane_events_[0]), "hipStreamWaitEvent");
            arena_lane_ = lane;
            enqueue_chunk(in, start, std::min(chunk_cap_, batch - start), ls);
        }
        arena_lane_ = 0;
        for (int l = 1; l < lanes_; l++) {
            hip_check(record_event(lane_events_[l], side_streams_[l - 1]), "hipEventRecord");
            hip_check(wait_event(s, lane_events_[l]), "hipStreamWaitEvent");
        }
        return;
    }
    int chunk = chunk_cap_;
    for (int start = 0; start < batch; start += chunk) enqueue_chunk(in, start, std::min(chunk, batch - start), s);
}

bool Model::takes_u8_input() {
    if (dirty_) rebuild();
    return mi::takes_u8_input(plan_, consts_);
}

// Test hook (option "test_poison"): every buffer a run may only read after writing it gets bytes no kernel should ever see — 0xFF (NaN) or 0x7F
// (3.39e38: survives max / ReLU, which drop a NaN). Enqueued on the run's stream, outside any graph, so it precedes the whole run on every lane and head
// stream (they all start behind an event on that stream). Left alone on purpose: weights, stage / tail / band programs, band constants, the band
// workspace and its generation (packet tags start from a cleared workspace: band_before_launch) — state by design, not scratch.
void Model::poison_scratch(hipStream_t s) {
    const int byte = test_poison_ == 1 ? 0xFF : 0x7F;
    if (d_arena_) hip_check(hipMemsetAsync(d_arena_, byte, std::max<size_t>(arena_floats_, 64) * sizeof(float), s), "hipMemsetAsync poison arena");
    if (d_small_) hip_check(hipMemsetAsync(d_small_, byte, small_floats_ * sizeof(float), s), "hipMemsetAsync poison small-batch scratch");
    for (int k = 0; k < static_cast<int>(d_out_.size()); k++)
        if (d_out_[k]) hip_check(hipMemsetAsync(d_out_[k], byte, output_elems(k) * sizeof(float) * batch_cap_, s), "hipMemsetAsync poison outputs");
}

void Model::run_device_u8(const uint8_t* frames, long frame_bytes, int row_bytes, const float* lut, int batch, hipStream_t stream) {
    if (batch <= 0) throw std::runtime_error("batch must be positive");
    if (!frames || !lut) throw std::runtime_error("null tensor pointer");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (!takes_u8_input()) throw std::runtime_error("plan: this graph has no u8 input form");
    ensure_capacity(batch);
    if (test_poison_) poison_scratch(stream ? stream : stream_);
    u8_.frames = frames; u8_.lut = lut; u8_.frame_bytes = frame_bytes; u8_.row_bytes = row_bytes;
    try {
        // the graph input tensor itself is never read: `in` only has to be a stable non-null key
        run_graph_or_eager(reinterpret_cast<const float*>(frames), batch, stream ? stream : stream_, GraphKey{frames, batch, frame_bytes, row_bytes});
    } catch (...) {
        u8_ = U8Input{};
        throw;
    }
    u8_ = U8Input{};
}

void Model::run_device(const float* in, int batch, hipStream_t stream, bool one_shot) {
    if (batch <= 0) throw std::runtime_error("batch must be positive");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (dirty_) rebuild();
    ensure_capacity(batch);
    band_use_ = band_usable(batch) && (band_ == 2 || one_shot);
    band_ran_ = band_use_;
    GraphKey key{in, batch, 0, 0};
    key.band = band_use_;
    hipStream_t s = stream ? stream : stream_;
    if (test_poison_) poison_scratch(s);
    if (band_use_) band_before_launch(s);
    try {
        run_graph_or_eager(in, batch, s, key);
    } catch (...) {
        band_use_ = false;
        throw;
    }
    const bool checked_here = band_use_ && !one_shot;
    band_use_ = false;
    if (checked_here) {
        // option band = 2 (tests, profiling, bench --opt): nobody behind this call asks band_failed(), so the run is checked here — a launch that gave
        // up leaves void results: wait for it and repeat the run on the batched plan
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (band_failed()) {
            key.band = false;
            run_graph_or_eager(in, batch, s, key);
        }
    }
}

// In front of every single-launch run: the packet tags are 64 x generation + stage + 1 in 32 bits, and the packet slots of frames a launch does not
// have keep their old tags — after 2^26 launches of a handle (hours of single-image calls) a stale packet could carry the tag a reader waits for.
// Well before that the workspace and the generation are cleared (behind everything the stream holds).
void Model::band_before_launch(hipStream_t s) {
    constexpr unsigned kWrap = (1u << 26) - 4096u;   // (Model::profile repeats a launch a few times per call)
    band_gen_ += static_cast<unsigned>(std::max(1, profile_inner_));
    if (band_gen_ < kWrap || !d_band_ws_) return;
    hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    hip_check(hipMemsetAsync(d_band_ws_, 0, band_ws_bytes_, s), "hipMemsetAsync band workspace");
    if (!band_gen_force_) hip_check(hipMemsetAsync(d_band_sync_, 0, 64 * sizeof(unsigned), s), "hipMemsetAsync band generation");
    else {   // test hook: the device's generation is moved to the same count, so that the real tags do wrap in the launches that follow
        const unsigned g[4] = {kWrap + 4096u - 2u, 0u, 0u, 0u};
        hip_check(hipMemcpyAsync(d_band_sync_, g, sizeof(g), hipMemcpyHostToDevice, s), "band generation");
        band_gen_force_ = false;
    }
    hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    band_gen_ = 0;
    band_wraps_++;
}

bool Model::band_usable(int batch) const {
    return band_plan_.ready && band_ > 0 && lanes_ == 1 && batch <= band_plan_.max_frames && batch <= chunk_cap_;
}

int Model::band_workgroups(int batch) {
    if (dirty_) rebuild();
    return band_plan_.ready && band_ > 0 && lanes_ == 1 && batch <= band_plan_.max_frames ? batch * band_plan_.nw : 0;
}

bool Model::band_failed() {
    if (band_test_fail_ && band_ran_) { band_test_fail_ = 0; band_ran_ = false; return true; }
    const bool ran = band_ran_;
    band_ran_ = false;
    if (!h_band_fail_ || !*h_band_fail_) {
        if (ran) band_fail_streak_ = 0;
        return false;
    }
    *h_band_fail_ = 0;
    // a handle whose single launches keep giving up (other processes' kernels on the CUs, a CU mask) stops trying: every failed call costs the
    // kernel's bounded wait on top of the batched plan it then runs anyway
    if (++band_fail_streak_ >= 3 && band_ > 0) {
        band_ = 0;
        band_disabled_ = true;
        invalidate_graphs();
    }
    return true;
}

void Model::run_graph_or_eager(const float* in, int batch, hipStream_t s, const GraphKey& key) {
    // A single-launch run that is two launches in all (first convolution + band program) goes out eagerly: replaying a two-node graph costs
    // more than it saves (tools/probes/graph_probe.py: FaceDetection::infer BackCamera 252 -> 242 us, Short 170 -> 160; with the face mesh's
    // two more launches behind the program the graph wins again, 191 against 200 us)
    const bool eager = !use_graph_ || (band_use_ && band_run_launches(plan_, band_plan_) <= 2);
    if (eager) {
        enqueue_all(in, batch, s);
        return;
    }
    auto it = graphs_.find(key);
    if (it == graphs_.end()) {
        if (graphs_.size() > 16) invalidate_graphs();
        // The plan becomes a hipGraph built node by node (launch.hpp) — no stream capture, which is process-wide runtime
        // state that other host threads break (and are broken by).
        GraphRecorder rec;
        hip_check(hipGraphCreate(&rec.graph, 0), "hipGraphCreate");
        current_recorder() = &rec;
        try {
            enqueue_all(in, batch, s);
        } catch (...) {
            current_recorder() = nullptr;
            hipGraphDestroy(rec.graph);
            throw;
        }
        current_recorder() = nullptr;
        hipGraphExec_t exec = nullptr;
        hipError_t e = hipGraphInstantiate(&exec, rec.graph, nullptr, nullptr, 0);
        hipGraphDestroy(rec.graph);
        hip_check(e, "hipGraphInstantiate");
        it = graphs_.emplace(key, exec).first;
    }
    hip_check(hipGraphLaunch(it->second, s), "hipGraphLaunch");
}

void Model::run(const float* in, int batch, float* const* outs, int mem, hipStream_t stream) {
    if (!in || !outs) throw std::runtime_error("null tensor pointer");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hipStream_t s = stream ? stream : stream_;
    const float* din = in;
    if (mem == 0) {
        size_t need = input_elems() * static_cast<size_t>(batch);
        if (need > in_stage_floats_) {
            invalidate_graphs();
            if (d_in_stage_) hip_check(hipFree(d_in_stage_), "hipFree stage");
            d_in_stage_ = nullptr;
            hip_check(hipMalloc(reinterpret_cast<void**>(&d_in_stage_), need * sizeof(float)), "hipMalloc stage");
            in_stage_floats_ = need;
        }
        hip_check(hipMemcpyAsync(d_in_stage_, in, need * sizeof(float), hipMemcpyHostToDevice, s), "H2D input");
        if (test_poison_ && in_stage_floats_ > need)   // the stage beyond this call's frames (a larger earlier call's)
            hip_check(hipMemsetAsync(d_in_stage_ + need, test_poison_ == 1 ? 0xFF : 0x7F, (in_stage_floats_ - need) * sizeof(float), s), "hipMemsetAsync poison stage");
        din = d_in_stage_;
    }
    run_device(din, batch, s);
    for (int k = 0; k < num_outputs(); k++) {
        if (!outs[k]) continue;
        hip_check(hipMemcpyAsync(outs[k], d_out_[k], output_elems(k) * sizeof(float) * batch,
                                 mem == 0 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s), "copy outputs");
    }
    if (mem == 0 || !stream) hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
}

size_t Model::debug_tensor(int tensor, int frame, float* dst, size_t cap) {
    const Graph& g = plan_.graph;
    if (tensor < 0 || tensor >= static_cast<int>(g.tensors.size())) throw std::runtime_error("tensor index out of range");
    if (frame < 0 || frame >= last_chunk_frames_) throw std::runtime_error("frame outside the last chunk");
    bool produced = false;
    for (const Node& n : plan_.nodes) produced |= (n.out == tensor);
    if (!produced) throw std::runtime_error("tensor was fused away (or is an input/constant)");
    long fs;
    float* p = tensor_ptr_mut(plan_, launch_ctx(nullptr, 0, last_chunk_frames_), tensor, &fs);
    size_t n = std::min(cap, g.tensors[tensor].elems());
    hip_check(hipDeviceSynchronize(), "sync");
    hip_check(hipMemcpy(dst, p + static_cast<long>(frame) * fs, n * sizeof(float), hipMemcpyDeviceToHost), "D2H debug");
    return n;
}

}  // namespace mi
