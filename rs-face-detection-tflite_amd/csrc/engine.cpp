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
constexpr int kHeadStreams = 4;  // most side streams for output heads that run beside the trunk (option "heads")

void same_pad(int in, int k, int stride, int out, int* before) { *before = std::max(0, (out - 1) * stride + k - in) / 2; }
long align_up(long v, long a) { return (v + a - 1) / a * a; }
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
           kBandGen = 128 }; // stored in band_gen_, and the next band launch takes the wrap path (band_gen_force_)
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
        {"stem_mfma", &Model::stem_mfma_, 0, 1, 0},  // 0: the detectors' 5x5 first convolution stays on stem_conv_kernel (packed VALU FMAs) at every batch size (bit-identical)
        {"pair_fuse", &Model::pair_fuse_, 0, 1, 0},  // 0: two plain blocks in a row keep a launch each (the face mesh's 48x48x32 blocks: mwalk_kernel), no mdblock_kernel<pair>
        {"mdb_band", &Model::mdb_band_, 0, 4096, 0},  // rows per band of the mdblock_kernel launches (0: chosen per launch)
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
    consts_ = pack_plan_consts(plan_);  // every constant the launches need and the stage programs (consts.cpp)
    upload(d_weights_, consts_.blob, "hipMalloc weights", "upload weights");  // (never empty: the blob ends in its slack)
    upload(d_tail_programs_, consts_.tail_progs, "hipMalloc programs", "upload programs");
    upload(d_programs_, consts_.progs, "hipMalloc programs", "upload programs");
    schedule_side_streams();
    build_bandnet();
    dirty_ = false;
    chunk_cap_ = 0;
}

// Output heads that may run beside the trunk: compute nodes whose output lives in a graph-output buffer and is
// read by no other launch, and that come after the last trunk node in plan order (so no later trunk launch can
// re-use arena memory they still read: the arena's liveness analysis follows plan order)
void Model::schedule_side_streams() {
    const Graph& g = plan_.graph;
    const size_t N = plan_.nodes.size();
    head_slot_.assign(N, -1); head_wait_.assign(N, -1); event_after_.assign(N, 0);
    auto is_view = [&](const Node& n) { return n.kind == Node::Reshape || n.kind == Node::Concat; };
    auto root = [&](int t) { return plan_.storage[t].root; };
    auto producer = [&](int t, size_t before) {  // the last launch in front of node `before` that writes (the buffer of) tensor t, -1: none
        int prod = -1;
        for (size_t j = 0; j < before; j++) {
            if (is_view(plan_.nodes[j])) continue;
            bool makes = root(plan_.nodes[j].out) == root(t);
            for (int x : plan_.nodes[j].extra_out) makes |= root(x) == root(t);
            if (makes) prod = static_cast<int>(j);
        }
        return prod;
    };
    auto beside = [&](size_t i, int slot, int prod) {  // node i runs on side stream `slot`, behind launch prod
        head_slot_[i] = slot % std::max(1, std::min(head_streams_opt_, kHeadStreams));
        head_wait_[i] = prod;
        if (prod >= 0) event_after_[static_cast<size_t>(prod)] = 1;
    };
    std::vector<int> out_roots;
    for (int o : g.outputs) out_roots.push_back(root(o));
    std::vector<char> head(N, 0);
    int last_trunk = -1;
    for (size_t i = 0; i < N; i++) {
        const Node& n = plan_.nodes[i];
        if (is_view(n)) continue;
        bool feeds_output = std::find(out_roots.begin(), out_roots.end(), root(n.out)) != out_roots.end();
        for (size_t j = 0; j < N && feeds_output; j++) {
            const Node& m = plan_.nodes[j];
            if (is_view(m)) continue;
            for (int x : m.in) if (x == n.out) feeds_output = false;
            if (m.res == n.out) feeds_output = false;
        }
        if (n.kind == Node::Resident && (n.in.size() != 1 || !n.extra_out.empty())) feeds_output = false;  // several inputs / outputs: stays on the trunk
        head[i] = feeds_output;
        if (!feeds_output) last_trunk = static_cast<int>(i);
    }
    int slots = 0;
    for (size_t i = 0; i < N; i++) {
        const Node& n = plan_.nodes[i];
        if (!head[i] || static_cast<int>(i) < last_trunk || is_view(n)) continue;
        if (n.res >= 0 && n.res != n.in[0]) continue;  // two producers: keep it on the trunk
        // heads are spread round robin over `heads` side streams (option, default 1).  They are independent of each other, but
        // on BackCamera (four small heads behind the last trunk launch) every extra parallel branch of the replay graph cost
        // more than it hid: 1.675 ms per step with 1 stream, 1.69 / 1.68 / 1.72 with 2 / 3 / 4
        beside(i, slots++, producer(n.in[0], i));
    }
    // tail branches (Plan::branch): chain 0 stays on the trunk stream, every other chain runs on a side stream behind the launch
    // that produced its newest input (the trunk runs in plan order, so the older inputs are done by then; launches of the same
    // chain share a stream).  The arena keeps everything the branches touch allocated to the end of the plan.
    static const bool no_branches = getenv("MI_NO_BRANCHES") != nullptr;  // development aid
    for (size_t i = 0; i < N && !no_branches && plan_.branch.size() == N; i++) {
        const Node& n = plan_.nodes[i];
        if (plan_.branch[i] < 1 || is_view(n)) continue;
        int prod = n.res >= 0 ? producer(n.res, i) : -1;
        for (int t : n.in) prod = std::max(prod, producer(t, i));
        beside(i, plan_.branch[i] - 1, prod);
    }
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

const float* Model::tensor_ptr(int t, const float* in, int chunk_start, long* fs) const {
    const Graph& g = plan_.graph;
    const Storage& s = plan_.storage[t];
    *fs = s.frame_stride;
    if (s.root == plan_.storage[g.inputs[0]].root) return in + static_cast<long>(chunk_start) * s.frame_stride + s.offset;
    return tensor_ptr_mut(t, chunk_start, fs);
}

float* Model::tensor_ptr_mut(int t, int chunk_start, long* fs) const {
    const Graph& g = plan_.graph;
    const Storage& s = plan_.storage[t];
    *fs = s.frame_stride;
    for (size_t k = 0; k < g.outputs.size(); k++)
        if (plan_.storage[g.outputs[k]].root == s.root) return d_out_[k] + static_cast<long>(chunk_start) * s.frame_stride + s.offset;
    if (s.root == plan_.storage[g.inputs[0]].root) throw std::runtime_error("plan writes into the graph input");
    long off = plan_.root_offset[s.root];
    if (off < 0) throw std::runtime_error("tensor has no storage");
    return d_arena_ + static_cast<size_t>(plan_.arena_floats_per_frame) * chunk_cap_ * arena_lane_ + off * chunk_cap_ + s.offset;
}

std::string Model::node_label(const Node& n) const {
    const Graph& g = plan_.graph;
    switch (n.kind) {
        case Node::Conv: return n.gemm_head ? "head_gemm_kernel" : "conv_generic_kernel";
        case Node::Dw: return "dw_kernel";
        case Node::Block: {
            const int Co = g.tensors[n.out].shape.back();
            const int MT = (Co + 31) / 32, MTG = std::min(4, MT), PG = MT <= 2 ? 2 : 1;
            return "block_kernel<" + std::to_string(MTG) + "," + std::to_string(n.w >= 0 ? n.sh : 1) + "," + (n.w >= 0 ? "3" : "1") + "," + std::to_string(PG) + ">";
        }
        case Node::Chain: {
            const auto& so = g.tensors[n.out].shape;
            if (n.chain_pre || n.chain_post) {
                const auto& sm = g.tensors[n.members[n.chain_pre ? 1 : 0].in[0]].shape;
                return "chain_kernel<" + std::to_string((sm.back() + 31) / 32) + ">";
            }
            if (g.tensors[n.in[0]].shape[1] * g.tensors[n.in[0]].shape[2] <= 256) return "chain_kernel<" + std::to_string((so.back() + 31) / 32) + ">";
            const auto& sin = g.tensors[n.in[0]].shape;
            const int nh2 = n.members.back().sh == 2 ? so.back() / sin.back() : 0;
            const int rps = strip_pipe_rows_per_step(sin[1], pipe_rows_);
            return std::string(rps == 4 ? "strip_pipe1m_kernel<" : (rps == 3 ? "strip_pipe2m_kernel<" : (rps == 2 ? "strip_pipe2_kernel<" : "strip_pipe_kernel<"))) + std::to_string(sin.back() / 4) + "," + std::to_string(n.members.size()) + "," + (n.members[0].act == ACT_RELU ? "1" : "0") + "," + std::to_string(nh2) + ">";
        }
        case Node::Resident: return n.xc ? "xc_kernel" : (n.dblock ? "dblock_kernel" : (n.bneck ? "bneck_kernel" : (n.tail ? "tail_kernel" : "resident_kernel")));
        case Node::Add: return "add_kernel";
        case Node::Act: return "act_kernel";
        case Node::MaxPool: return "maxpool_kernel";
        case Node::Pad: return "pad_kernel";
        case Node::Resize: return "resize_kernel";
        case Node::DepthToSpace: return "d2s_kernel";
        default: return "view";
    }
}

std::vector<Model::LaunchStat> Model::profile(const float* in, int batch, int reps, hipStream_t stream) {
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (dirty_) rebuild();
    const int saved_chunk = chunk_;
    ensure_capacity(batch);
    hipStream_t s = stream ? stream : stream_;
    const Graph& g = plan_.graph;
    std::vector<LaunchStat> stats;
    for (const Node& n : plan_.nodes) {
        if (n.kind == Node::Reshape || n.kind == Node::Concat) continue;
        LaunchStat st;
        st.kernel = node_label(n);
        auto elems = [&](int t) { return t >= 0 ? static_cast<double>(g.tensors[t].elems()) : 0.0; };
        double per_frame = 4 * elems(n.out);
        for (int t : n.in) per_frame += 4 * elems(t);
        if (n.res >= 0 && !(n.kind == Node::Block && n.res == n.in[0])) per_frame += 4 * elems(n.res);
        double weights = 0;
        for (int c : {n.w, n.b, n.w2, n.b2, n.alpha}) weights += 4 * elems(c);
        st.bytes = per_frame * batch + weights;
        const auto& si = g.tensors[n.in[0]].shape;
        const auto& so = g.tensors[n.out].shape;
        if (n.kind == Node::Conv) st.macs = elems(n.out) * n.KH * n.KW * si.back() * batch;
        if (n.kind == Node::Dw) st.macs = elems(n.out) * n.KH * n.KW * batch;
        if (n.kind == Node::Block) st.macs = elems(n.out) / so.back() * si.back() * ((n.w >= 0 ? 9 : 0) + so.back()) * batch;
        if (n.kind == Node::Resident) {
            st.macs = 0;
            for (int t : n.extra_out) st.bytes += 4 * elems(t) * batch;
            for (const Node& m : n.members) {
                const auto& mo = g.tensors[m.out].shape;
                const int Cm = g.tensors[m.in[0]].shape[3];
                if (m.kind == Node::Conv) st.macs += elems(m.out) * m.KH * m.KW * Cm * batch;
                else st.macs += static_cast<double>(mo[1]) * mo[2] * Cm * ((m.w >= 0 ? 9 : 0) + mo[3]) * batch;
                for (int c : {m.w, m.b, m.w2, m.b2, m.alpha}) st.bytes += 4 * elems(c);
            }
        }
        if (n.kind == Node::Chain) {
            st.macs = 0;
            for (int t : n.extra_out) st.bytes += 4 * elems(t) * batch;
            for (const Node& m : n.members) {
                const auto& mo = g.tensors[m.out].shape;
                st.macs += static_cast<double>(mo[1]) * mo[2] * g.tensors[m.in[0]].shape[3] * (9 + mo[3]) * batch;
            }
            for (const Node& m : n.members)
                for (int c : {m.w, m.b, m.w2, m.b2, m.alpha}) st.bytes += 4 * elems(c);
            for (const Node& m : n.head_nodes) {
                st.macs += elems(m.out) * g.tensors[m.in[0]].shape[3] * batch;
                for (int c : {m.w, m.b, m.w2, m.b2}) st.bytes += 4 * elems(c);
            }
        }
        std::string d;
        for (size_t k = 1; k < si.size(); k++) d += (k > 1 ? "x" : "") + std::to_string(si[k]);
        d += "->";
        for (size_t k = 1; k < so.size(); k++) d += (k > 1 ? "x" : "") + std::to_string(so[k]);
        st.detail = d;
        stats.push_back(st);
    }
    const size_t nl = stats.size();
    const int nchunks = (batch + chunk_cap_ - 1) / chunk_cap_;
    std::vector<hipEvent_t> marks;
    // one untimed pass first: the first launch of a kernel symbol in a process loads its code object (about a millisecond,
    // which averaged over a few reps made the first layer of every kernel type look 3x slower than its twins)
    profile_inner_ = 4;
    band_use_ = band_ == 2 && band_usable(batch);
    for (int r = -1; r < reps; r++) {
        marks.clear();
        std::vector<std::string> labels;
        for (int start = 0; start < batch; start += chunk_cap_) enqueue_chunk(in, start, std::min(chunk_cap_, batch - start), s, &marks, &labels);
        for (size_t i = 0; i < nl && i < labels.size(); i++) stats[i].kernel = labels[i];
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (marks.size() != static_cast<size_t>(nchunks) * (nl + 1)) throw std::runtime_error("internal: profile marks mismatch");
        for (int c = 0; c < nchunks; c++)
            for (size_t i = 0; i < nl; i++) {
                float ms = 0;
                hip_check(hipEventElapsedTime(&ms, marks[c * (nl + 1) + i], marks[c * (nl + 1) + i + 1]), "hipEventElapsedTime");
                if (r >= 0) stats[i].ms += ms / reps / profile_inner_;
            }
        for (hipEvent_t ev : marks) hipEventDestroy(ev);
    }
    profile_inner_ = 1;
    band_use_ = false;
    (void)saved_chunk;
    // plan nodes that ran inside the launch before them (a run of blocks on mstrip_chain_kernel): their work belongs to that launch
    for (size_t i = 1; i < stats.size();) {
        if (stats[i].kernel == "(inside the band launch)") {   // its work belongs to the band launch, which need not be the entry in front of it
            for (size_t j = 0; j < i; j++)
                if (stats[j].kernel == "bandnet_kernel") {
                    stats[j].ms += stats[i].ms; stats[j].bytes += stats[i].bytes; stats[j].macs += stats[i].macs;
                    const size_t arrow = stats[i].detail.find("->"), parrow = stats[j].detail.find("->");
                    if (arrow != std::string::npos && parrow != std::string::npos) stats[j].detail = stats[j].detail.substr(0, parrow) + stats[i].detail.substr(arrow);
                }
            stats.erase(stats.begin() + static_cast<long>(i));
        } else if (stats[i].kernel == "(fused into previous launch)") {
            stats[i - 1].ms += stats[i].ms; stats[i - 1].bytes += stats[i].bytes; stats[i - 1].macs += stats[i].macs;
            const size_t arrow = stats[i].detail.find("->");
            const size_t parrow = stats[i - 1].detail.find("->");
            if (arrow != std::string::npos && parrow != std::string::npos) stats[i - 1].detail = stats[i - 1].detail.substr(0, parrow) + stats[i].detail.substr(arrow);
            stats.erase(stats.begin() + static_cast<long>(i));
        } else {
            i++;
        }
    }
    return stats;
}

void Model::enqueue_chunk(const float* in, int chunk_start, int F, hipStream_t s, std::vector<hipEvent_t>* marks,
                          std::vector<std::string>* labels) {
    const Graph& g = plan_.graph;
    auto mark = [&] {
        if (!marks) return;
        hipEvent_t ev;
        hip_check(hipEventCreate(&ev), "hipEventCreate");
        hip_check(hipEventRecord(ev, s), "hipEventRecord");  // profiling marks: eager launches only
        marks->push_back(ev);
    };
    mark();
    // heads beside the trunk (not while profiling: the per-launch events there assume one stream)
    // (with several lanes the chunks already overlap; the head streams and node events are one set per model, and sharing
    // them between concurrently captured lanes crashes hipGraph capture)
    const bool fork = fork_ && !marks && lanes_ == 1;
    hipStream_t const trunk = s;
    unsigned used_heads = 0;
    auto node_event = [&](size_t k) {
        if (head_events_.size() < plan_.nodes.size() + 2 + kHeadStreams) head_events_.resize(plan_.nodes.size() + 2 + kHeadStreams, nullptr);
        if (!head_events_[k]) hip_check(hipEventCreateWithFlags(&head_events_[k], hipEventDisableTiming), "hipEventCreate");
        return head_events_[k];
    };
    int fused_behind = 0;   // plan nodes that ran inside the launch just made (a run of 32x32x48 blocks on mstrip_chain_kernel)
    const bool band = band_use_ && chunk_start == 0;
    for (size_t i = 0; i < plan_.nodes.size(); i++) {
        const Node& n = plan_.nodes[i];
        if (n.kind == Node::Reshape || n.kind == Node::Concat) continue;  // views
        if (band && static_cast<int>(i) >= band_plan_.first && !band_plan_.node_runs[i]) {
            // the single-launch plan: everything behind the first convolution is this one launch (bandnet_kernels.hip), but for the nodes behind
            // the program's end (band_plan_.node_runs), which keep their launches
            if (static_cast<int>(i) > band_plan_.first) {
                if (labels) labels->push_back("(inside the band launch)");
                mark();
                continue;
            }
            if (labels) labels->push_back("bandnet_kernel");
            BandLaunch a;
            a.prog = d_band_prog_; a.nstages = band_plan_.nstages; a.NW = band_plan_.nw; a.F = F; a.lds_bytes = band_plan_.lds_bytes;
            a.tiles_floats = band_plan_.tiles_floats;
            a.dw_floats = band_plan_.dw_floats; a.ws_frame_floats = band_plan_.ws_frame_floats;
            long fs = 0;
            a.base[0] = d_band_ws_;
            a.base[1] = const_cast<float*>(tensor_ptr(band_plan_.stem_out, in, chunk_start, &fs));
            a.cv2 = band_plan_.cv2 ? 1 : 0;
            a.xb = band_plan_.xb ? 1 : 0;
            a.wide = band_plan_.wide ? 1 : 0;
            for (size_t k = 0; k < band_plan_.ext.size(); k++) {
                long efs = 0;
                a.base[2 + k] = band_plan_.ext[k].out_k >= 0 ? d_out_[static_cast<size_t>(band_plan_.ext[k].out_k)] : tensor_ptr_mut(band_plan_.ext[k].tensor, chunk_start, &efs);
            }
            a.consts = d_band_consts_; a.sync = d_band_sync_; a.fail = d_band_fail_;
            a.absent_mod = band_test_absent_;
            int rc = 0;
            for (int rep_ = 0; rep_ < (marks ? profile_inner_ : 1) && rc == 0; rep_++) rc = launch_bandnet(a, trunk);
            if (rc != 0) throw std::runtime_error(std::string("kernel launch failed: ") + hipGetErrorString(static_cast<hipError_t>(rc)));
            // launches behind the program that run beside the trunk wait for the node that made their input: every such node inside the
            // program is this launch
            for (size_t j = i; fork && j < plan_.nodes.size(); j++)
                if (!band_plan_.node_runs[j] && event_after_[j]) hip_check(record_event(node_event(j), trunk), "hipEventRecord");
            mark();
            continue;
        }
        if (fused_behind > 0) {
            fused_behind--;
            if (labels) labels->push_back("(fused into previous launch)");
            if (fork && event_after_[i]) hip_check(record_event(node_event(i), trunk), "hipEventRecord");
            mark();
            continue;
        }
        s = trunk;
        // (a whole-frame convolution right behind the band launch stays on the trunk: the face mesh's two heads are 9 + 11 us, a side stream's
        // events cost more than they hide — FaceLandmark::infer 208 us forked, 190 us in line)
        const bool in_line = band && n.gemm_head && head_wait_[i] >= 0 && !band_plan_.node_runs[static_cast<size_t>(head_wait_[i])];
        if (fork && head_slot_[i] >= 0 && !in_line) {
            while (static_cast<int>(head_streams_.size()) <= head_slot_[i]) {
                hipStream_t st;
                hip_check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
                head_streams_.push_back(st);
            }
            s = head_streams_[head_slot_[i]];
            if (head_wait_[i] >= 0) {
                hip_check(wait_event(s, node_event(static_cast<size_t>(head_wait_[i]))), "hipStreamWaitEvent");
            } else {  // reads the graph input: order it behind whatever the trunk stream was doing before this plan
                hip_check(record_event(node_event(plan_.nodes.size()), trunk), "hipEventRecord");
                hip_check(wait_event(s, node_event(plan_.nodes.size())), "hipStreamWaitEvent");
            }
            used_heads |= 1u << head_slot_[i];
        }
        const auto& si = g.tensors[n.in[0]].shape;
        const auto& so = g.tensors[n.out].shape;
        auto dim = [](const std::vector<int>& v, size_t d) { return d < v.size() ? v[d] : 1; };
        Epilogue ep;
        ep.bias = (n.kind == Node::Block ? consts_.node_b2[i] : consts_.node_b[i]) >= 0 ? d_weights_ + (n.kind == Node::Block ? consts_.node_b2[i] : consts_.node_b[i]) : nullptr;
        ep.alpha = consts_.node_alpha[i] >= 0 ? d_weights_ + consts_.node_alpha[i] : nullptr;
        ep.act = n.act;
        if (n.res >= 0) {
            const auto& sr = g.tensors[n.res].shape;
            ep.res = tensor_ptr(n.res, in, chunk_start, &ep.res_fs);
            ep.res_mode = n.res_mode;
            ep.res_after = n.res_after ? 1 : 0;
            ep.res_C = sr.back();
            ep.res_H = dim(sr, 1);
            ep.res_W = dim(sr, 2);
        }
        int rc = 0;
        long in_fs = 0, out_fs = 0;
        if (labels) labels->push_back(node_label(n));
        const float* ip = tensor_ptr(n.in[0], in, chunk_start, &in_fs);
        float* op = tensor_ptr_mut(n.out, chunk_start, &out_fs);
        // profiling: the launch is repeated between its two marks (a launch never reads what it writes), so that the event bubble
        // between marks is shared by profile_inner_ executions and the per-launch figure approaches rocprofv3's kernel duration
        for (int rep_ = 0; rep_ < (marks ? profile_inner_ : 1) && rc == 0; rep_++)
        switch (n.kind) {
            case Node::Conv: {
                if (n.gemm_head) {
                    HeadGemmArgs h;
                    h.in = ip; h.out = op; h.in_fs = in_fs; h.out_fs = out_fs;
                    h.w = d_weights_ + consts_.node_w[i];
                    h.bias = ep.bias; h.alpha = ep.alpha; h.act = ep.act;
                    h.B = F; h.K = si[1] * si[2] * si[3]; h.N = so[3];
                    rc = launch_head_gemm(h, s);
                    if (labels) labels->back() = F <= 4 ? "head_dot_kernel" : "head_gemm_kernel";   // (launch_head_gemm: a handful of frames take the dot-product form)
                    break;
                }
                // the first convolution inside the launch of the pair of BlazeBlocks behind it (f32 pictures, from 32 frames on: mdblock_kernels.hip, MD::STEM)
                if (strip_ && stem_fuse_ && consts_.node_stem[i] >= 0 && !u8_.frames) {   // (consts_.node_stem: the graph's side of the conditions, checked when the constants were packed)
                    const size_t j = i + 1;
                    if (consts_.node_chain_pair[j] >= 0 && !event_after_[i] && head_slot_[j] < 0) {
                        const Node& c = plan_.nodes[j];
                        const auto& co = g.tensors[c.out].shape;
                        DblockArgs d;
                        long ofs = 0;
                        d.out = tensor_ptr_mut(c.out, chunk_start, &ofs); d.out_fs = ofs;
                        d.B = F; d.H = so[1]; d.W = so[2]; d.C = so[3]; d.Cm = g.tensors[c.members[0].out].shape[3]; d.Co = co[3];
                        d.hi1 = c.members[0].act == ACT_RELU6 ? 6.f : INFINITY;
                        d.hi2 = c.members[1].act == ACT_RELU6 ? 6.f : INFINITY;
                        d.skip1 = 1; d.skip2_from_a = 1;
                        d.act1 = c.members[0].act; d.act2 = c.members[1].act;
                        d.mconsts = d_weights_ + consts_.node_chain_pair[j];
                        d.stem_in = ip; d.stem_in_fs = in_fs; d.stem_consts = d_weights_ + consts_.node_stem[i];
                        d.stem_hi = n.act == ACT_RELU6 ? 6.f : INFINITY;
                        d.band_rows = mdb_band_;
                        if (mdblock_kernel_supports(d)) {
                            if (labels) labels->back() = "mdblock_kernel<stem+pair>";
                            rc = launch_mdblock(d, s);
                            fused_behind = 1;
                            break;
                        }
                    }
                }
                ConvArgs a;
                a.in = ip; a.out = op; a.in_fs = in_fs; a.out_fs = out_fs;
                a.w = d_weights_ + consts_.node_w[i];
                a.B = F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.Ho = so[1]; a.Wo = so[2]; a.Co = so[3]; a.Cop = (a.Co + 3) & ~3;
                a.KH = n.KH; a.KW = n.KW; a.sh = n.sh; a.sw = n.sw;
                if (n.padding == Padding::Same) { same_pad(a.H, a.KH, a.sh, a.Ho, &a.pt); same_pad(a.W, a.KW, a.sw, a.Wo, &a.pl); }
                if (n.ept >= 0) { a.pt = n.ept; a.pl = n.epl; }
                a.ep = ep;
                a.no_mfma = stem_mfma_ ? 0 : 1;
                if (u8_.frames && plan_.storage[n.in[0]].root == plan_.storage[g.inputs[0]].root) {
                    if (!conv_takes_u8(a)) throw std::runtime_error("plan: this graph's first convolution has no u8 input form");
                    a.in_u8 = u8_.frames + static_cast<long>(chunk_start) * u8_.frame_bytes;
                    a.u8_lut = u8_.lut; a.u8_frame_bytes = u8_.frame_bytes; a.u8_row_bytes = u8_.row_bytes;
                }
                if (labels) labels->back() = conv_kernel_label(a);
                rc = launch_conv(a, s);
                break;
            }
            case Node::Dw: {
                DwArgs a;
                a.in = ip; a.out = op; a.in_fs = in_fs; a.out_fs = out_fs;
                a.w = d_weights_ + consts_.node_w[i];
                a.B = F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.Ho = so[1]; a.Wo = so[2];
                a.KH = n.KH; a.KW = n.KW; a.sh = n.sh; a.sw = n.sw;
                if (n.padding == Padding::Same) { same_pad(a.H, a.KH, a.sh, a.Ho, &a.pt); same_pad(a.W, a.KW, a.sw, a.Wo, &a.pl); }
                if (n.ept >= 0) { a.pt = n.ept; a.pl = n.epl; }
                a.ep = ep;
                rc = launch_dw(a, s);
                break;
            }
            case Node::Resident: {
                if (n.xc) {
                    XcArgs a;
                    a.in = ip; a.in_fs = in_fs; a.out = op; a.out_fs = out_fs;
                    a.B = F; a.H = si[1]; a.W = si[2]; a.nstages = static_cast<int>(n.members.size());
                    for (size_t k = 0; k < n.members.size(); k++) {
                        const Node& m = n.members[k];
                        const MemberOff& mo = consts_.chain_off[i][k];
                        XcStage& st = a.st[k];
                        st.cblob = d_weights_ + mo.cblob;
                        st.has_dw = m.w >= 0;
                        st.w_pw = d_weights_ + mo.w2;
                        st.C = g.tensors[m.in[0]].shape[3]; st.Co = g.tensors[m.out].shape[3]; st.act = m.act;
                        st.skip = m.res < 0 ? 0 : (m.res == m.in[0] ? 1 : (k >= 2 && m.res == n.members[k - 2].out ? 3 : 2));
                        if (st.skip == 2) {
                            st.res = tensor_ptr(m.res, in, chunk_start, &st.res_fs);
                            st.res_C = g.tensors[m.res].shape[3]; st.res_W = g.tensors[m.res].shape[2];
                        }
                    }
                    rc = launch_xc(a, s);
                    break;
                }
                if (n.dblock) {
                    DblockArgs a;
                    a.in = ip; a.in_fs = in_fs; a.out = op; a.out_fs = out_fs;
                    a.B = F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.Cm = g.tensors[n.members[0].out].shape[3]; a.Co = so[3];
                    a.w1 = d_weights_ + consts_.chain_off[i][0].w2;
                    a.w2 = d_weights_ + consts_.chain_off[i][1].w2;
                    a.consts = d_weights_ + consts_.chain_off[i][0].cblob;
                    a.hi1 = n.members[0].act == ACT_RELU6 ? 6.f : INFINITY;
                    a.hi2 = n.members[1].act == ACT_RELU6 ? 6.f : INFINITY;
                    a.skip1 = n.members[0].res >= 0;                       // two plain BlazeBlocks: each adds its own input
                    a.skip2_from_a = n.members[1].res == n.members[0].out;
                    a.act1 = n.members[0].act; a.act2 = n.members[1].act;
                    if (consts_.chain_off[i][1].mconsts >= 0) a.mconsts = d_weights_ + consts_.chain_off[i][1].mconsts;
                    if (strip_ && mdblock_kernel_supports(a)) {
                        if (labels) labels->back() = "mdblock_kernel";
                        rc = launch_mdblock(a, s);
                        break;
                    }
                    rc = launch_dblock(a, s);
                    break;
                }
                if (n.bneck) {
                    BneckArgs a;
                    a.in = ip; a.in_fs = in_fs; a.out = op; a.out_fs = out_fs;
                    a.B = F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.Cm = g.tensors[n.members[0].out].shape[3];
                    a.nblocks = static_cast<int>(n.members.size() / 2);
                    a.bands = n.res_bands;
                    for (int k = 0; k < a.nblocks; k++) {
                        const MemberOff &ma = consts_.chain_off[i][static_cast<size_t>(2 * k)], &mb = consts_.chain_off[i][static_cast<size_t>(2 * k + 1)];
                        a.blocks[k].w1 = d_weights_ + ma.w2;
                        a.blocks[k].w2 = d_weights_ + mb.w2;
                        a.blocks[k].consts = d_weights_ + ma.cblob;
                        a.blocks[k].hi1 = n.members[static_cast<size_t>(2 * k)].act == ACT_RELU6 ? 6.f : INFINITY;
                        a.blocks[k].hi2 = n.members[static_cast<size_t>(2 * k + 1)].act == ACT_RELU6 ? 6.f : INFINITY;
                        a.blocks[k].act1 = n.members[static_cast<size_t>(2 * k)].act;
                        a.blocks[k].act2 = n.members[static_cast<size_t>(2 * k + 1)].act;
                        if (mb.mconsts >= 0) a.blocks[k].mconsts = d_weights_ + mb.mconsts;
                    }
                    if (strip_ && mbneck_kernel_supports(a)) {
                        if (labels) labels->back() = "mbneck_kernel";
                        rc = launch_mbneck(a, s);
                        break;
                    }
                    rc = launch_bneck(a, s);
                    break;
                }
                if (n.tail) {
                    TailLaunch a;
                    a.prog = d_tail_programs_ + consts_.node_prog[i];
                    a.nstages = static_cast<int>(n.stages.size());
                    a.B = F;
                    a.frame_floats = n.tail_frame_floats;
                    a.variant = tail_pre_;
                    // frames per workgroup: as many as keep every CU busy (a workgroup's stage costs the same few thousand cycles of
                    // latency whether its pixel tiles are full or not), within what the CU's LDS holds
                    const int gmax = std::max(1, (160 * 1024 - 1024) / (4 * n.tail_frame_floats));
                    a.G = tail_g_ > 0 ? std::min(tail_g_, gmax) : std::max(1, std::min(gmax, F / device_cu_count()));
                    for (int k = 0; k < kResBases; k++) { a.bases.p[k] = nullptr; a.bases.scale[k] = 0; a.bases.frame0[k] = 0; }
                    a.bases.p[0] = d_arena_ + static_cast<size_t>(plan_.arena_floats_per_frame) * chunk_cap_ * arena_lane_;
                    a.bases.scale[0] = chunk_cap_;
                    a.bases.p[1] = const_cast<float*>(in);
                    a.bases.frame0[1] = chunk_start;
                    for (int k = 0; k < num_outputs() && 2 + k < kResBases; k++) { a.bases.p[2 + k] = d_out_[k]; a.bases.frame0[2 + k] = chunk_start; }
                    a.bases.weights = d_weights_;
                    rc = launch_tail(a, s);
                    break;
                }
                ResLaunch a;
                a.prog = d_programs_ + consts_.node_prog[i];
                a.nstages = static_cast<int>(n.stages.size());
                a.B = F;
                a.bands = n.res_bands;
                a.const_off = n.res_const_off;
                a.const_floats = n.res_const_floats;
                a.lds_bytes = n.res_lds_bytes;
                for (int k = 0; k < kResBases; k++) { a.bases.p[k] = nullptr; a.bases.scale[k] = 0; a.bases.frame0[k] = 0; }
                a.bases.p[0] = d_arena_ + static_cast<size_t>(plan_.arena_floats_per_frame) * chunk_cap_ * arena_lane_;
                a.bases.scale[0] = chunk_cap_;
                a.bases.p[1] = const_cast<float*>(in);
                a.bases.frame0[1] = chunk_start;
                for (int k = 0; k < num_outputs() && 2 + k < kResBases; k++) { a.bases.p[2 + k] = d_out_[k]; a.bases.frame0[2 + k] = chunk_start; }
                a.bases.weights = d_weights_;
                rc = launch_resident(a, s);
                break;
            }
            case Node::Chain: {
                ChainArgs a;
                auto fill = [&](ChainBlock& cb, size_t k) {
                    const MemberOff& mo = consts_.chain_off[i][k];
                    cb.w_dw = d_weights_ + mo.w;
                    cb.b_dw = mo.b >= 0 ? d_weights_ + mo.b : nullptr;
                    cb.w_pw = d_weights_ + mo.w2;
                    cb.bias = mo.b2 >= 0 ? d_weights_ + mo.b2 : nullptr;
                    cb.alpha = mo.alpha >= 0 ? d_weights_ + mo.alpha : nullptr;
                    cb.act = n.members[k].act;
                    cb.has_res = n.members[k].res >= 0;
                };
                if (n.chain_pre || n.chain_post || !n.head_pairs.empty()) {  // frame-resident chain with stride-2 blocks around it and / or output heads in the same launch
                    const size_t k0 = n.chain_pre ? 1 : 0, k1 = n.members.size() - (n.chain_post ? 1 : 0);
                    const auto& sm = g.tensors[n.members[k0].in[0]].shape;  // the resident frame
                    a.B = F; a.H = sm[1]; a.W = sm[2]; a.C = sm[3]; a.nblocks = static_cast<int>(k1 - k0);
                    for (size_t k = k0; k < k1; k++) fill(a.blocks[k - k0], k);
                    const int t_main = n.members[k1 - 1].out;   // the chain's own output tensor
                    a.write_out = n.out == t_main || std::find(n.extra_out.begin(), n.extra_out.end(), t_main) != n.extra_out.end();
                    if (a.write_out) { a.out = tensor_ptr_mut(t_main, chunk_start, &a.out_fs); } else { a.out = op; a.out_fs = out_fs; }
                    if (n.chain_pre) {
                        a.pre.on = 1; fill(a.pre.blk, 0);
                        a.pre.in = ip; a.pre.in_fs = in_fs; a.pre.Cin = si[3];
                        a.in = ip; a.in_fs = in_fs;
                    } else {
                        a.in = ip; a.in_fs = in_fs;
                    }
                    if (n.chain_post) {
                        const int t_post = n.members.back().out;
                        a.post.on = 1; fill(a.post.blk, n.members.size() - 1);
                        a.post.out = tensor_ptr_mut(t_post, chunk_start, &a.post.out_fs);
                        a.post.Co = g.tensors[t_post].shape[3];
                    }
                    for (size_t k = 0; k < n.head_pairs.size(); k++) {
                        const Node::HeadPair& hp = n.head_pairs[k];
                        ChainHead& H = a.heads[hp.src];
                        H.on = 1; H.src = hp.src;
                        H.w_pw = d_weights_ + consts_.chain_head_off[i][k].w2;
                        H.bias = d_weights_ + consts_.chain_head_off[i][k].b2;
                        const int ta = n.head_nodes[static_cast<size_t>(hp.a)].out;
                        H.Co_a = g.tensors[ta].shape.back();
                        H.out_a = tensor_ptr_mut(ta, chunk_start, &H.out_a_fs);
                        if (hp.b >= 0) {
                            const int tb = n.head_nodes[static_cast<size_t>(hp.b)].out;
                            H.Co_b = g.tensors[tb].shape.back();
                            H.out_b = tensor_ptr_mut(tb, chunk_start, &H.out_b_fs);
                        }
                    }
                    if (!chain_kernel_supports(a)) throw std::runtime_error("chain node with edge stages without a kernel");
                    rc = launch_chain(a, s);
                    break;
                }
                a.in = ip; a.out = op; a.in_fs = in_fs; a.out_fs = out_fs;
                a.B = F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.nblocks = static_cast<int>(n.members.size());
                if (a.nblocks <= kMaxChain && a.H * a.W <= 256 && chain_kernel_supports(a)) {  // frame-resident in LDS
                    for (size_t k = 0; k < n.members.size(); k++) fill(a.blocks[k], k);
                    rc = launch_chain(a, s);
                    break;
                }
                if (strip_ && consts_.node_chain_pair[i] >= 0) {   // a pair of plain BlazeBlocks with an operand-layout form
                    DblockArgs d;
                    d.in = ip; d.in_fs = in_fs; d.out = op; d.out_fs = out_fs;
                    d.B = F; d.H = si[1]; d.W = si[2]; d.C = si[3]; d.Cm = g.tensors[n.members[0].out].shape[3]; d.Co = so[3];
                    d.hi1 = n.members[0].act == ACT_RELU6 ? 6.f : INFINITY;
                    d.hi2 = n.members[1].act == ACT_RELU6 ? 6.f : INFINITY;
                    d.skip1 = 1; d.skip2_from_a = 1;
                    d.act1 = n.members[0].act; d.act2 = n.members[1].act;
                    d.mconsts = d_weights_ + consts_.node_chain_pair[i];
                    d.band_rows = mdb_band_;
                    if (mdblock_kernel_supports(d)) {
                        if (labels) labels->back() = "mdblock_kernel<pair>";
                        rc = launch_mdblock(d, s);
                        break;
                    }
                }
                // row-pipelined group of strip blocks: only the first input and the last output exist in memory
                std::vector<BlockArgs> blk(n.members.size());
                for (size_t k = 0; k < n.members.size(); k++) {
                    const MemberOff& mo = consts_.chain_off[i][k];
                    const Node& m = n.members[k];
                    BlockArgs& b = blk[k];
                    b.in = ip; b.out = op; b.in_fs = in_fs; b.out_fs = out_fs;
                    b.has_dw = 1;
                    b.pipe_rows = pipe_rows_;
                    b.pipe_band = pipe_band_;
                    b.w_dw = d_weights_ + mo.w;
                    b.b_dw = mo.b >= 0 ? d_weights_ + mo.b : nullptr;
                    b.w_pw = d_weights_ + mo.w2;
                    b.w_strip = mo.strip >= 0 ? d_weights_ + mo.strip : nullptr;
                    b.B = F; b.H = si[1]; b.W = si[2]; b.C = si[3]; b.Ho = si[1]; b.Wo = si[2]; b.Co = si[3];
                    b.sh = b.sw = 1; b.pt = b.pl = 1;
                    b.ep.bias = mo.b2 >= 0 ? d_weights_ + mo.b2 : nullptr;
                    b.ep.alpha = mo.alpha >= 0 ? d_weights_ + mo.alpha : nullptr;
                    b.ep.act = m.act;
                    if (m.res >= 0) { b.ep.res = b.in; b.ep.res_fs = b.in_fs; b.ep.res_C = b.C; b.ep.res_mode = RES_DIRECT; }
                    if (m.sh == 2) {  // stride-2 tail: halves the resolution, 2x2 max-pool skip from its (never materialised) input
                        b.sh = b.sw = 2; b.pt = b.pl = 0;
                        b.Ho = so[1]; b.Wo = so[2]; b.Co = so[3];
                        if (m.res >= 0) { b.ep.res_mode = RES_MAXPOOL; b.ep.res_H = b.H; b.ep.res_W = b.W; }
                    }
                }
                // Small batches: a row pipeline is a chain of 2S + rows/2 dependent steps of ~5 us whatever the batch (88 us per launch for ONE
                // BackCamera frame, four such launches of its 0.6 ms), while one strip-kernel launch per block is hundreds of independent
                // waves (~5 us).  Below `small_chain_` frames the members run one launch each, ping-ponging through a per-handle scratch.
                if (small_chain_ > 0 && F <= small_chain_ && lanes_ == 1 && d_small_) {
                    const int nb = static_cast<int>(blk.size());
                    const long fsz = static_cast<long>(si[1]) * si[2] * si[3];
                    float* T[2] = {d_small_, d_small_ + static_cast<size_t>(small_chain_) * fsz};
                    std::vector<BlockArgs> sb = blk;
                    const float* cur = ip;
                    long cur_fs = in_fs;
                    bool ok = static_cast<size_t>(2 * small_chain_) * fsz <= small_floats_;
                    for (int k = 0; k < nb && ok; k++) {
                        BlockArgs& b = sb[static_cast<size_t>(k)];
                        b.in = cur; b.in_fs = cur_fs;
                        if (b.ep.res_mode != RES_NONE) { b.ep.res = cur; b.ep.res_fs = cur_fs; }
                        if (k == nb - 1) { b.out = op; b.out_fs = out_fs; } else { b.out = T[k & 1]; b.out_fs = fsz; }
                        ok = b.sh == 1 ? strip_kernel_supports(b) : block_kernel_supports(b);   // (the stride-2 member too, or the run fails where the row pipeline below would have taken it)
                        cur = b.out; cur_fs = b.out_fs;
                    }
                    if (ok) {
                        if (labels) {
                            char name[48], buf[112];
                            const bool s2 = sb[static_cast<size_t>(nb - 1)].sh == 2;
                            snprintf(buf, sizeof buf, "%s x%d%s (small batch)", strip_kernel_label(sb[0], name, sizeof name), s2 ? nb - 1 : nb, s2 ? " + block_kernel" : "");
                            labels->back() = buf;
                        }
                        for (int k = 0; k < nb && rc == 0; k++) rc = sb[static_cast<size_t>(k)].sh == 1 ? launch_strip(sb[static_cast<size_t>(k)], s) : launch_block(sb[static_cast<size_t>(k)], s);
                        break;
                    }
                }
                if (!strip_pipe_supports(blk.data(), static_cast<int>(blk.size()))) throw std::runtime_error("chain node without a kernel");
                if (labels) { char buf[96]; labels->back() = strip_pipe_label(blk.data(), static_cast<int>(blk.size()), buf, sizeof buf); }
                rc = launch_strip_pipe(blk.data(), static_cast<int>(blk.size()), s);
                break;
            }
            case Node::Block: {
                BlockArgs a;
                a.in = ip; a.out = op; a.in_fs = in_fs; a.out_fs = out_fs;
                a.has_dw = n.w >= 0;
                a.w_dw = a.has_dw ? d_weights_ + consts_.node_w[i] : nullptr;
                a.b_dw = consts_.node_b[i] >= 0 ? d_weights_ + consts_.node_b[i] : nullptr;
                a.w_pw = d_weights_ + consts_.node_w2[i];
                a.B = F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.Ho = so[1]; a.Wo = so[2]; a.Co = so[3];
                a.sh = n.sh; a.sw = n.sw;
                if (a.has_dw && n.padding == Padding::Same) { same_pad(a.H, 3, a.sh, a.Ho, &a.pt); same_pad(a.W, 3, a.sw, a.Wo, &a.pl); }
                if (a.has_dw && n.ept >= 0) { a.pt = n.ept; a.pl = n.epl; }
                a.ep = ep;
                a.w_strip = consts_.node_strip[i] >= 0 ? d_weights_ + consts_.node_strip[i] : nullptr;
                a.w_mwalk = consts_.node_mwalk[i] >= 0 ? d_weights_ + consts_.node_mwalk[i] : nullptr;
                // this block and the next one as ONE launch (mdblock_kernel, pair form): the tensor between them is neither written nor read
                if (strip_ && pair_fuse_ && consts_.node_pair[i] >= 0 && i + 1 < plan_.nodes.size() && !event_after_[i] && head_slot_[i + 1] < 0 && head_slot_[i] < 0) {
                    const Node& nb = plan_.nodes[i + 1];
                    {
                        DblockArgs d;
                        long ofs = 0;
                        d.in = ip; d.in_fs = in_fs;
                        d.out = tensor_ptr_mut(nb.out, chunk_start, &ofs); d.out_fs = ofs;
                        d.B = F; d.H = si[1]; d.W = si[2]; d.C = si[3]; d.Cm = si[3]; d.Co = si[3];
                        d.hi1 = n.act == ACT_RELU6 ? 6.f : INFINITY;
                        d.hi2 = nb.act == ACT_RELU6 ? 6.f : INFINITY;
                        d.skip1 = 1; d.skip2_from_a = 1;
                        d.act1 = n.act; d.act2 = nb.act;
                        d.mconsts = d_weights_ + consts_.node_pair[i];
                        d.band_rows = mdb_band_;
                        // (the launch reads its input while it writes its output: the arena keeps the two apart — plan.cpp, liveness — and this checks it)
                        const bool apart = d.out + d.out_fs * F <= d.in || d.in + d.in_fs * F <= d.out;
                        if (apart && mdblock_kernel_supports(d)) {
                            if (labels) labels->back() = "mdblock_kernel<pair>";
                            rc = launch_mdblock(d, s);
                            fused_behind = 1;
                            break;
                        }
                    }
                }
                if (strip_ && ms2_kernel_supports(a)) {
                    if (labels) { char buf[96]; labels->back() = ms2_kernel_label(a, buf, sizeof buf); }
                    rc = launch_ms2(a, s);
                    break;
                }
                if (strip_ && mwalk_kernel_supports(a)) {
                    if (labels) { char buf[96]; labels->back() = mwalk_kernel_label(a, buf, sizeof buf); }
                    rc = launch_mwalk(a, s);
                    break;
                }
                const bool strip = strip_ && strip_kernel_supports(a);
                const bool mstrip = strip_ && !strip && mstrip_kernel_supports(a);
                if (mstrip && mchain_ && lanes_ == 1) {
                    // the blocks behind this one that the same kernel takes, each reading its predecessor's output: ONE launch for the run
                    // (every intermediate tensor keeps its arena slot; a workgroup per frame walks through the blocks)
                    std::vector<BlockArgs> run{a};
                    for (size_t j = i + 1; j < plan_.nodes.size() && run.size() < 8; j++) {
                        const Node& m = plan_.nodes[j];
                        if (m.kind != Node::Block || m.w < 0 || m.in.size() != 1 || m.in[0] != plan_.nodes[j - 1].out || consts_.node_strip[j] < 0 || head_slot_[j] >= 0) break;
                        const auto& mi_ = g.tensors[m.in[0]].shape;
                        const auto& mo_ = g.tensors[m.out].shape;
                        if (mi_.size() != 4 || mo_ != mi_) break;
                        BlockArgs bb;
                        bb.in = tensor_ptr(m.in[0], in, chunk_start, &bb.in_fs);
                        bb.out = tensor_ptr_mut(m.out, chunk_start, &bb.out_fs);
                        bb.has_dw = 1;
                        bb.w_dw = d_weights_ + consts_.node_w[j];
                        bb.b_dw = consts_.node_b[j] >= 0 ? d_weights_ + consts_.node_b[j] : nullptr;
                        bb.w_pw = d_weights_ + consts_.node_w2[j];
                        bb.w_strip = d_weights_ + consts_.node_strip[j];
                        bb.B = F; bb.H = mi_[1]; bb.W = mi_[2]; bb.C = mi_[3]; bb.Ho = mo_[1]; bb.Wo = mo_[2]; bb.Co = mo_[3];
                        bb.sh = m.sh; bb.sw = m.sw;
                        if (m.padding == Padding::Same) { same_pad(bb.H, 3, bb.sh, bb.Ho, &bb.pt); same_pad(bb.W, 3, bb.sw, bb.Wo, &bb.pl); }
                        if (m.ept >= 0) break;
                        bb.ep.bias = consts_.node_b2[j] >= 0 ? d_weights_ + consts_.node_b2[j] : nullptr;
                        bb.ep.alpha = consts_.node_alpha[j] >= 0 ? d_weights_ + consts_.node_alpha[j] : nullptr;
                        bb.ep.act = m.act;
                        if (m.res >= 0) {
                            if (m.res != m.in[0] || m.res_mode != RES_DIRECT || m.res_after) break;
                            bb.ep.res = bb.in; bb.ep.res_fs = bb.in_fs; bb.ep.res_mode = RES_DIRECT; bb.ep.res_C = bb.C;
                            bb.ep.res_H = bb.H; bb.ep.res_W = bb.W;
                        }
                        run.push_back(bb);
                        if (!mstrip_chain_supports(run.data(), static_cast<int>(run.size()))) { run.pop_back(); break; }
                    }
                    if (run.size() >= 2) {
                        if (labels) { char buf[96]; snprintf(buf, sizeof buf, "mstrip_chain_kernel<%d,%d>", a.C / 4, a.ep.act == ACT_RELU ? 1 : 0); labels->back() = buf; }
                        rc = launch_mstrip_chain(run.data(), static_cast<int>(run.size()), s);
                        fused_behind = static_cast<int>(run.size()) - 1;
                        break;
                    }
                }
                if (labels) { char buf[96]; labels->back() = strip ? strip_kernel_label(a, buf, sizeof buf) : (mstrip ? mstrip_kernel_label(a, buf, sizeof buf) : block_kernel_label(a, buf, sizeof buf)); }
                rc = strip ? launch_strip(a, s) : (mstrip ? launch_mstrip(a, s) : launch_block(a, s));
                break;
            }
            default: {
                EltArgs a;
                a.a = ip; a.a_fs = in_fs; a.out = op; a.out_fs = out_fs; a.alpha = ep.alpha; a.act = n.act;
                a.B = F; a.H = dim(si, 1); a.W = dim(si, 2); a.C = si.back();
                a.Ho = dim(so, 1); a.Wo = dim(so, 2); a.Co = so.back();
                if (si.size() != 4) { a.H = 1; a.W = 1; a.C = static_cast<int>(g.tensors[n.in[0]].elems()); a.Ho = a.Wo = 1; a.Co = a.C; }
                if (n.kind == Node::Add) {
                    a.b = tensor_ptr(n.in[1], in, chunk_start, &a.b_fs);
                    rc = launch_add(a, s);
                } else if (n.kind == Node::Act) {
                    rc = launch_act(a, s);
                } else if (n.kind == Node::MaxPool) {
                    a.p0 = n.filter_h; a.p1 = n.filter_w; a.p2 = n.sh; a.p3 = n.sw;
                    rc = launch_maxpool(a, s);
                } else if (n.kind == Node::Pad) {
                    const auto& pv = g.tensors[n.pads].i32;
                    if (pv[0] != 0 || pv[1] != 0) throw std::runtime_error("PAD on the batch axis unsupported");
                    a.p0 = pv[2]; a.p1 = pv[4]; a.p2 = pv[6];
                    rc = launch_padc(a, s);
                } else if (n.kind == Node::Resize) {
                    a.p0 = n.half_pixel; a.p1 = n.align_corners;
                    rc = launch_resize2x(a, s);
                } else if (n.kind == Node::DepthToSpace) {
                    a.p0 = n.block_size;
                    rc = launch_depth_to_space(a, s);
                } else {
                    throw std::runtime_error("internal: unhandled node kind");
                }
            }
        }
        if (rc != 0) throw std::runtime_error(std::string("kernel launch failed: ") + hipGetErrorString(static_cast<hipError_t>(rc)));
        if (fork && event_after_[i]) hip_check(record_event(node_event(i), s), "hipEventRecord");
        mark();
    }
    s = trunk;
    for (int k = 0; k < kHeadStreams; k++)  // join: the trunk stream continues (post-processing, the next chunk) after every head
        if (used_heads & (1u << k)) {
            hip_check(record_event(node_event(plan_.nodes.size() + 1 + k), head_streams_[static_cast<size_t>(k)]), "hipEventRecord");
            hip_check(wait_event(trunk, node_event(plan_.nodes.size() + 1 + k)), "hipStreamWaitEvent");
        }
    last_chunk_frames_ = F;
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
    const Graph& g = plan_.graph;
    const int root = plan_.storage[g.inputs[0]].root;
    int readers = 0;
    bool stem = false;
    for (const Node& n : plan_.nodes) {
        if (n.kind == Node::Reshape || n.kind == Node::Concat) continue;
        bool reads = false;
        for (int t : n.in) reads |= t >= 0 && plan_.storage[t].root == root;
        if (n.res >= 0 && plan_.storage[n.res].root == root) reads = true;
        if (!reads) continue;
        readers++;
        if (n.kind == Node::Conv && !n.gemm_head && n.in[0] >= 0 && plan_.storage[n.in[0]].root == root) {
            const auto& si = g.tensors[n.in[0]].shape;
            const auto& so = g.tensors[n.out].shape;
            ConvArgs a;
            a.out = reinterpret_cast<float*>(uintptr_t{256}); a.out_fs = 4;  // aligned placeholders: only the shape tests matter here
            a.C = si[3]; a.Co = so[3]; a.KH = n.KH; a.KW = n.KW; a.sh = n.sh; a.sw = n.sw;
            static const float some_bias = 0.f;
            a.ep.bias = &some_bias;
            a.ep.res_mode = n.res >= 0 ? n.res_mode : RES_NONE;
            stem = conv_takes_u8(a) && consts_.node_b[&n - plan_.nodes.data()] >= 0;
        }
    }
    return readers == 1 && stem;
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
    bool eager = !use_graph_;
    if (band_use_ && !eager) {
        int launches = 1;
        for (size_t i = 0; i < plan_.nodes.size(); i++) {
            const Node& n = plan_.nodes[i];
            if (n.kind == Node::Reshape || n.kind == Node::Concat) continue;
            if (static_cast<int>(i) < band_plan_.first || band_plan_.node_runs[i]) launches++;
        }
        eager = launches <= 2;
    }
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
    const Storage& st = plan_.storage[tensor];
    bool produced = false;
    for (const Node& n : plan_.nodes) produced |= (n.out == tensor);
    if (!produced) throw std::runtime_error("tensor was fused away (or is an input/constant)");
    long fs;
    float* p = tensor_ptr_mut(tensor, 0, &fs);
    size_t n = std::min(cap, g.tensors[tensor].elems());
    hip_check(hipDeviceSynchronize(), "sync");
    hip_check(hipMemcpy(dst, p + static_cast<long>(frame) * fs, n * sizeof(float), hipMemcpyDeviceToHost), "D2H debug");
    (void)st;
    return n;
}

}  // namespace mi
