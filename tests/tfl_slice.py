"""Stand-alone .tflite slices of the shipped graphs, cut at launch boundaries (test infrastructure).

The hand-written kernels are otherwise compared with a reference only at the outputs of whole networks, where the layers behind a launch attenuate
and mix what it got wrong.  A slice is one launch's worth of operators (or as many consecutive launches as it takes for the slice to lower like its
parent) written out as a model of its own: nothing stands between the launch and the comparison, its input can be chosen, and a failure names it.

slice_graph() reads a graph with oracle/np/tfl3.py, keeps the operators between one activation tensor and a set of output tensors, turns the
DEQUANTIZE / DENSIFY constants into dense f32 constants (exact: f16 -> f32 widening) and writes the result with synth_tflite's flatbuffer writer.
CHAINS / EXTRA are the table of cuts per shipped graph, made with `launches_dump tensors` (tests/launches_dump.cpp), THERE_FOR the launch labels
each slice is there for, and NOT_COVERED the launch labels no slice reaches.  tests/test_slices_cpu.py checks both on the CPU; tests/test_f64_parity_gpu.py runs them.
"""
import numpy as np

import synth_tflite as st
from oracle.np import evaluate, tfl3

# BuiltinOptions union tags of the operators synth_tflite does not write (tensorflow/lite/schema/schema.fbs)
OPT_RESIZE_BILINEAR, OPT_DEPTH_TO_SPACE = 15, 94


def _producers(graph):
    return {o: op for op in graph.ops for o in op.outputs}


def _const_value(graph, prod, i):
    """Tensor i as a dense constant (f32, or i32 for shapes / paddings), or None when it is an activation."""
    t = graph.tensors[i]
    if t.data is not None:
        if t.sparsity is not None:
            return None          # only DENSIFY reads it
        a = np.asarray(t.data).reshape(t.shape if t.shape else ())
        return a.astype(np.float32) if a.dtype == np.float16 else a
    op = prod.get(i)
    if op is None:
        return None
    if op.code == tfl3.DENSIFY:
        return evaluate.densify(graph.tensors[op.inputs[0]]).astype(np.float32)
    if op.code == tfl3.DEQUANTIZE:
        src = _const_value(graph, prod, op.inputs[0])
        return None if src is None else src.astype(np.float32)
    return None


def slice_graph(graph, tensor_in, tensors_out):
    """The operators of `graph` between activation `tensor_in` and the activations `tensors_out`, as the bytes of a .tflite file whose input is
    tensor_in and whose outputs are tensors_out, in that order.  ValueError when an output depends on an activation other than tensor_in."""
    prod = _producers(graph)
    need, seen, stack = set(), set(), list(tensors_out)
    while stack:
        t = stack.pop()
        if t in seen or t == tensor_in or t < 0:
            continue
        seen.add(t)
        if _const_value(graph, prod, t) is not None:
            continue
        op = prod.get(t)
        if op is None:
            raise ValueError("tensor %d (%s) is an activation that does not follow from tensor %d" % (t, graph.tensors[t].name, tensor_in))
        need.add(op.index)
        stack.extend(op.inputs)
    if tensor_in in tensors_out or not need:
        raise ValueError("empty slice")
    shape_in = list(graph.tensors[tensor_in].shape)
    gb = st.GraphBuilder(0, shape_in)
    ids = {tensor_in: gb.input}

    def tid(i):
        if i < 0:
            return -1
        if i not in ids:
            c = _const_value(graph, prod, i)
            assert c is not None, i
            ids[i] = gb.const(c, graph.tensors[i].name, dtype=0 if c.dtype == np.float32 else 2)
        return ids[i]

    for op in graph.ops:
        if op.index not in need:
            continue
        c, o, opts = op.code, op.opts, None
        tag = 0
        ins = list(op.inputs)
        if c == tfl3.CONV_2D:
            assert o.get("dil_w", 1) == 1 and o.get("dil_h", 1) == 1
            tag, opts = st.OPT_CONV, [("i8", o["padding"]), ("i32", o["stride_w"]), ("i32", o["stride_h"]), ("i8", o["act"])]
        elif c == tfl3.DEPTHWISE_CONV_2D:
            assert o.get("dil_w", 1) == 1 and o.get("dil_h", 1) == 1
            tag, opts = st.OPT_DW, [("i8", o["padding"]), ("i32", o["stride_w"]), ("i32", o["stride_h"]), ("i32", o["depth_multiplier"]), ("i8", o["act"])]
        elif c == tfl3.MAX_POOL_2D:
            tag, opts = st.OPT_POOL, [("i8", o["padding"]), ("i32", o["stride_w"]), ("i32", o["stride_h"]), ("i32", o["filter_w"]), ("i32", o["filter_h"]),
                                      ("i8", o["act"])]
        elif c == tfl3.ADD:
            tag, opts = st.OPT_ADD, [("i8", o.get("act", 0))]
        elif c == tfl3.CONCATENATION:
            tag, opts = st.OPT_CONCAT, [("i32", o["axis"]), ("i8", o["act"])]
        elif c == tfl3.RESHAPE:
            shape = list(graph.tensors[op.outputs[0]].shape)
            tag, opts = st.OPT_RESHAPE, [("ints", shape)]
            ins = ins[:1]
        elif c == tfl3.PAD:
            tag, opts = st.OPT_PAD, []
        elif c == tfl3.RESIZE_BILINEAR:
            tag, opts = OPT_RESIZE_BILINEAR, [None, None, ("u8", int(o["align_corners"])), ("u8", int(o["half_pixel_centers"]))]
        elif c == tfl3.DEPTH_TO_SPACE:
            tag, opts = OPT_DEPTH_TO_SPACE, [("i32", o["block_size"])]
        elif c not in (tfl3.RELU, tfl3.PRELU):
            raise ValueError("operator %s inside a slice" % op.name)
        new_in = [tid(i) for i in ins]
        if c == tfl3.RESHAPE:
            new_in.append(gb.const(np.array(graph.tensors[op.outputs[0]].shape), "shape", dtype=2))
        assert len(op.outputs) == 1
        t = graph.tensors[op.outputs[0]]
        ids[op.outputs[0]] = gb._act(list(t.shape), t.name)
        gb.ops.append((c, new_in, [ids[op.outputs[0]]], tag, opts))
    gb.outputs = [ids[t] for t in tensors_out]
    return gb.finish()


# ---- the table of slices
# CHAINS: per shipped graph the cut tensors of its chain of slices: slice k runs from cut k to cut k + 1, the last one to the graph's outputs; fed one
# into the next the slices of a chain are the whole network.  The cuts are the boundaries of the launches in the default (fuse 5) launch list at 32
# frames (`launches_dump tensors`), the first slice starts at the graph input, and a slice holds one launch or as many consecutive launches as it needs
# to lower like its parent:
#   - a fused pair whose second block is the slice's output does not fuse (landmark: mdblock_kernel<stem+pair> / <pair> need the ms2 block behind them),
#     and the last block of an mstrip_chain run that is the slice's output runs on mstrip_kernel (back: the run ends at the chain launch's slice);
#   - the front / short-range detectors' tensors of 28 .. 88 channels are widened with zero channels by the lowering (plan_widen.cpp), which a slice's
#     input cannot be: their cuts are at the 24-channel tensors only;
#   - full / sparse: from the second stride-2 block on the pyramid's laterals keep earlier tensors alive, no single tensor separates the graph until the
#     last lateral is merged (84 -> 342, 131 -> 523).
CHAINS = {
    "back": [0, 4, 36, 69, 101, 136],
    "front": [0, 4, 12],
    "short": [0, 4, 12],
    "full": [0, 4, 19, 34, 52, 67, 84, 342, 357],
    "sparse": [0, 7, 32, 57, 69, 81, 106, 131, 523, 548],
    "landmark": [0, 35, 65, 74, 83],
    "iris": [0, 5, 19, 33, 47, 61, 78, 134, 149],
}
# EXTRA: slices beside the chains, (tensor_in, tensors_out or None for the graph's outputs): a launch of a longer chain slice on its own, so that a
# failure names it (back's chain launch with its six views; the face mesh's two stride-2 MFMA blocks), and back's 32x32x48 run ending in the
# slice's output (mstrip_chain_kernel for six blocks and the stand-alone mstrip_kernel for the seventh)
EXTRA = {
    "back": [(136, [192]), (192, None)],
    "landmark": [(23, [35]), (53, [65])],
}


def slice_id(name, tensor_in, tensors_out):
    return "%s:%d-%s" % (name, tensor_in, tensors_out[0] if tensors_out else "out")


def table(name):
    """[(id, tensor_in, tensors_out or None, in the chain)] of one shipped graph."""
    cuts = CHAINS[name]
    rows = [(cuts[k], [cuts[k + 1]] if k + 1 < len(cuts) else None, True) for k in range(len(cuts))]
    rows += [(tin, touts, False) for tin, touts in EXTRA.get(name, [])]
    return [(slice_id(name, tin, touts), tin, touts, chain) for tin, touts, chain in rows]


ALL_IDS = [row[0] for name in CHAINS for row in table(name)]

# THERE_FOR: slice -> (the parent's launch labels at 32 frames, at 1 frame) the slice is there for; tests/test_slices_cpu.py checks that the slice's own
# launch list holds each of them, template arguments and all, and that every label of every parent's list is some slice's
_BACK_PIPE, _BACK_SMALL = "strip_pipe2m_kernel<6,4,1,%d>", "strip_kernel<6,1> x%s (small batch)"
_PYRAMID_1 = ["block_kernel<1,1,1,1,0>", "block_kernel<1,1,1,1,1>", "block_kernel<1,1,3,1,0>", "block_kernel<1,1,3,1,1>", "block_kernel<1,2,3,1,0>",
              "block_kernel<1,2,3,1,1>", "dblock_kernel", "resident_kernel", "xc_kernel"]
_PYRAMID_32 = ["block_kernel<1,1,1,1,1>", "block_kernel<1,1,3,1,0>", "block_kernel<1,1,3,1,1>", "block_kernel<1,2,3,1,0>", "block_kernel<1,2,3,1,1>",
               "block_kernel<2,1,1,1,0>", "block_kernel<2,1,1,1,1>", "dblock_kernel", "resident_kernel", "xc_kernel"]
_DETECTOR_REST = (["block_kernel<1,1,3,2,0>", "block_kernel<2,2,3,1,0>", "chain_kernel<3>", "mstrip_chain_kernel<12,1>"],
                  ["block_kernel<1,1,3,1,0>", "block_kernel<1,2,3,1,0>", "chain_kernel<3>"])
THERE_FOR = {
    "back:0-4": (["stem_mfma_kernel"], ["stem_mfma_kernel"]),
    "back:4-36": ([_BACK_PIPE % 0], [_BACK_SMALL % "4"]),
    "back:36-69": ([_BACK_PIPE % 1], [_BACK_SMALL % "3 + block_kernel"]),
    "back:69-101": ([_BACK_PIPE % 0], [_BACK_SMALL % "4"]),
    "back:101-136": ([_BACK_PIPE % 2], [_BACK_SMALL % "3 + block_kernel"]),
    "back:136-out": (["chain_kernel<3>", "mstrip_chain_kernel<12,1>"], ["block_kernel<1,1,3,1,0>", "chain_kernel<3>"]),
    "back:136-192": (["mstrip_chain_kernel<12,1>"], ["block_kernel<1,1,3,1,0>"]),
    "back:192-out": (["chain_kernel<3>"], ["chain_kernel<3>"]),
    "front:0-4": (["stem_mfma_kernel"], ["stem_mfma_kernel"]),
    "front:4-12": (["strip_kernel<6,1>"], ["strip_kernel<6,1>"]),
    "front:12-out": _DETECTOR_REST,
    "short:0-4": (["stem_mfma_kernel"], ["stem_mfma_kernel"]),
    "short:4-12": (["strip_kernel<6,1>"], ["strip_kernel<6,1>"]),
    "short:12-out": _DETECTOR_REST,
    "full:0-4": (["stem_conv_kernel"], ["stem_conv_kernel"]),
    "full:4-19": (["mdblock_kernel"], ["dblock_kernel"]),
    "full:19-34": (["mdblock_kernel"], ["dblock_kernel"]),
    "full:34-52": (["block_kernel<2,1,3,1,1>", "ms2_kernel<8,1,3>"], ["block_kernel<1,1,3,1,1>", "block_kernel<1,2,3,1,0>"]),
    "full:52-67": (["mdblock_kernel"], ["dblock_kernel"]),
    "full:67-84": (["mdblock_kernel"], ["dblock_kernel"]),
    "full:84-342": (_PYRAMID_32 + ["block_kernel<3,1,3,1,1>", "ms2_kernel<16,2,2>"], _PYRAMID_1),
    "full:342-357": (["mdblock_kernel"], ["dblock_kernel"]),
    "full:357-out": (["block_kernel<1,1,1,1,0>", "pw_few_kernel"], ["block_kernel<1,1,1,1,0>", "pw_few_kernel"]),
    "sparse:0-7": (["stem_conv_kernel"], ["stem_conv_kernel"]),
    "sparse:7-32": (["mdblock_kernel"], ["dblock_kernel"]),
    "sparse:32-57": (["mdblock_kernel"], ["dblock_kernel"]),
    "sparse:57-69": (["block_kernel<1,2,3,1,0>"], ["block_kernel<1,2,3,1,0>"]),
    "sparse:69-81": (["block_kernel<2,1,3,2,0>"], ["block_kernel<1,1,3,1,0>"]),
    "sparse:81-106": (["dblock_kernel"], ["dblock_kernel"]),
    "sparse:106-131": (["dblock_kernel"], ["dblock_kernel"]),
    "sparse:131-523": (_PYRAMID_32 + ["block_kernel<4,1,3,1,0>"], _PYRAMID_1),
    "sparse:523-548": (["mdblock_kernel"], ["dblock_kernel"]),
    "sparse:548-out": (["block_kernel<1,1,1,1,0>", "block_kernel<2,1,1,1,0>", "d2s_kernel", "dw_kernel"], ["block_kernel<1,1,1,1,0>", "d2s_kernel", "dw_kernel"]),
    "landmark:0-35": (["mdblock_kernel<stem+pair>", "ms2_kernel<4,2,3>"], ["block_kernel<1,2,3,1,0>", "stem_conv_kernel", "strip_kernel<4,0> x2 (small batch)"]),
    "landmark:35-65": (["mdblock_kernel<pair>", "ms2_kernel<8,4,2>"], ["block_kernel<1,2,3,1,0>", "strip_kernel<8,0>"]),
    "landmark:65-74": (["block_kernel<2,1,3,1,0>"], ["block_kernel<1,1,3,1,0>"]),
    "landmark:74-83": (["block_kernel<2,1,3,1,0>"], ["block_kernel<1,1,3,1,0>"]),
    "landmark:83-out": (["head_gemm_kernel", "tail_kernel"], ["head_dot_kernel", "tail_kernel"]),
    "landmark:23-35": (["ms2_kernel<4,2,3>"], ["block_kernel<1,2,3,1,0>"]),
    "landmark:53-65": (["ms2_kernel<8,4,2>"], ["block_kernel<1,2,3,1,0>"]),
    "iris:0-5": (["stem_conv_kernel"], ["stem_conv_kernel"]),
    "iris:5-19": (["mbneck_kernel"], ["bneck_kernel"]),
    "iris:19-33": (["mbneck_kernel"], ["bneck_kernel"]),
    "iris:33-47": (["mbneck_kernel"], ["bneck_kernel"]),
    "iris:47-61": (["mbneck_kernel"], ["bneck_kernel"]),
    "iris:61-78": (["resident_kernel"], ["resident_kernel"]),
    "iris:78-134": (["bneck_kernel"], ["bneck_kernel"]),
    "iris:134-149": (["resident_kernel"], ["resident_kernel"]),
    "iris:149-out": (["head_gemm_kernel", "tail_kernel"], ["head_dot_kernel", "tail_kernel"]),
}
# NOT_COVERED: graph -> {launch label of its default list at 1 or 32 frames that no slice runs: why, read from the lowering}.  None: every label of
# the seven parents' lists is in the list of the slice THERE_FOR assigns it to.
NOT_COVERED = {}
