// render_kernels.hip — render_to_image (/root/reference/src/face_detection_lite/render.rs:361-479) on the device, for a batch.
//
// Two phases on one stream:
//   canvas  to_rgba8 (render.rs:365): RGB -> RGBA with alpha 255 (or RGB -> RGB).  Memory-bound; every thread moves 16 pixels
//           with 16-byte loads and stores where the rows of both pictures are 16-byte aligned, 4 pixels with dwords where they
//           are 4-byte aligned, single bytes otherwise; the pixels of a row behind its last full group go byte by byte.
//   draw    one workgroup per frame.  Annotations in list order with a fence and a workgroup barrier between two of them, which
//           is the reference's overwrite order: inside one annotation every item writes the same value, so its items are drawn
//           by lanes in parallel (one lane per line, a group of lanes per point square / filled rectangle).
//
// The arithmetic is the reference's, literally (include/mi_face.h, "render.rs"): f64 scaling, Rust `as` casts, u32 wrapping
// for the point squares, imageproc 0.25.0's BresenhamLineIter / draw_filled_rect_mut / draw_hollow_rect_mut.  Two deviations,
// both counted in skipped[frame]:
//   1. a rectangle whose of_size width or height is 0 is not drawn (imageproc panics);
//   2. a line's work is bounded by the canvas, not by its length: the steps in front of the canvas are skipped in closed form.
//      With E = 2 * error the walk is  E0 = dx;  per step E -= 2 dy, and if E < 0 { minor += step; E += 2 dx }  so after k
//      steps E = (dx - 2 dy k) mod 2 dx and the minor axis has moved -floor((dx - 2 dy k) / 2 dx) times.  This equals the f32
//      walk while every f32 value of it is exact: |coordinate| <= 2^20 after the i32 cast makes dx, dy and every error
//      half-integers below 2^23.  A line with an end point beyond 2^20 — a hollow rectangle with an edge beyond it — is not
//      drawn (the reference would walk up to 2^32 steps).
// Every pixel write is bounds-checked against the canvas, as imageproc's is.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "render.hpp"

namespace mi {
namespace {

constexpr int kDrawThreads = 256;

// face_landmark.rs:35-166 FACE_LANDMARK_CONNECTIONS (124 pairs), in the reference's order: lips (outer lower, outer upper,
// inner lower, inner upper), left eye (lower, upper), left eyebrow (lower, upper), right eye, right eyebrow, face oval.
__constant__ uint16_t kFaceConnections[124][2] = {
    {61, 146}, {146, 91}, {91, 181}, {181, 84}, {84, 17}, {17, 314}, {314, 405}, {405, 321}, {321, 375}, {375, 291},
    {61, 185}, {185, 40}, {40, 39}, {39, 37}, {37, 0}, {0, 267}, {267, 269}, {269, 270}, {270, 409}, {409, 291},
    {78, 95}, {95, 88}, {88, 178}, {178, 87}, {87, 14}, {14, 317}, {317, 402}, {402, 318}, {318, 324}, {324, 308},
    {78, 191}, {191, 80}, {80, 81}, {81, 82}, {82, 13}, {13, 312}, {312, 311}, {311, 310}, {310, 415}, {415, 308},
    {33, 7}, {7, 163}, {163, 144}, {144, 145}, {145, 153}, {153, 154}, {154, 155}, {155, 133},
    {33, 246}, {246, 161}, {161, 160}, {160, 159}, {159, 158}, {158, 157}, {157, 173}, {173, 133},
    {46, 53}, {53, 52}, {52, 65}, {65, 55},
    {70, 63}, {63, 105}, {105, 66}, {66, 107},
    {263, 249}, {249, 390}, {390, 373}, {373, 374}, {374, 380}, {380, 381}, {381, 382}, {382, 362},
    {263, 466}, {466, 388}, {388, 387}, {387, 386}, {386, 385}, {385, 384}, {384, 398}, {398, 362},
    {276, 283}, {283, 282}, {282, 295}, {295, 285},
    {300, 293}, {293, 334}, {334, 296}, {296, 336},
    {10, 338}, {338, 297}, {297, 332}, {332, 284}, {284, 251}, {251, 389}, {389, 356}, {356, 454}, {454, 323}, {323, 361},
    {361, 288}, {288, 397}, {397, 365}, {365, 379}, {379, 378}, {378, 400}, {400, 377}, {377, 152}, {152, 148}, {148, 176},
    {176, 149}, {149, 150}, {150, 136}, {136, 172}, {172, 58}, {58, 132}, {132, 93}, {93, 234}, {234, 127}, {127, 162},
    {162, 21}, {21, 54}, {54, 103}, {103, 67}, {67, 109}, {109, 10},
};
// iris_landmark.rs:44-60 EYE_LANDMARK_CONNECTIONS (15 pairs); MAX_EYE_LANDMARK = 15 (iris_landmark.rs:62)
__constant__ uint8_t kEyeConnections[15][2] = {
    {0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {6, 7}, {7, 8}, {9, 10}, {10, 11}, {11, 12}, {12, 13}, {13, 14}, {0, 9}, {8, 14},
};
constexpr int kFaceConnectionCount = 124, kEyeConnectionCount = 15, kEyeContourPoints = 15, kEyeRows = 76;

// ------------------------------------------------------------------------------------------------------------ canvas phase
// 12 bytes (4 RGB pixels, little-endian dwords a, b, c) -> 4 RGBA dwords
__device__ __forceinline__ uint4 rgb4_to_rgba(uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t A = 0xFF000000u;
    return make_uint4((a & 0x00FFFFFFu) | A, (((a >> 24) | (b << 8)) & 0x00FFFFFFu) | A, (((b >> 16) | (c << 16)) & 0x00FFFFFFu) | A, (c >> 8) | A);
}

// PX pixels per thread (16: uint4 accesses, 4: dwords, 1: bytes), OC bytes per output pixel
template <int PX, int OC>
__global__ __launch_bounds__(256) void render_canvas_kernel(RenderCanvas cv, int groups_per_row) {
    const long unit = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int y = static_cast<int>(unit / groups_per_row);
    if (y >= cv.height) return;
    const int x0 = static_cast<int>(unit - static_cast<long>(y) * groups_per_row) * PX;
    const int b = blockIdx.y;
    const uint8_t* src = cv.frames + (static_cast<long>(b) * cv.height + y) * cv.stride + 3L * x0;
    uint8_t* dst = cv.out + (static_cast<long>(b) * cv.height + y) * cv.out_stride + static_cast<long>(OC) * x0;
    if (PX > 1 && x0 + PX <= cv.width) {
        if (PX == 16) {
            const uint4* s = reinterpret_cast<const uint4*>(src);
            const uint4 v0 = s[0], v1 = s[1], v2 = s[2];
            uint4* d = reinterpret_cast<uint4*>(dst);
            if (OC == 4) {
                d[0] = rgb4_to_rgba(v0.x, v0.y, v0.z);
                d[1] = rgb4_to_rgba(v0.w, v1.x, v1.y);
                d[2] = rgb4_to_rgba(v1.z, v1.w, v2.x);
                d[3] = rgb4_to_rgba(v2.y, v2.z, v2.w);
            } else {
                d[0] = v0; d[1] = v1; d[2] = v2;
            }
        } else {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
            const uint32_t a = s[0], bb = s[1], c = s[2];
            uint32_t* d = reinterpret_cast<uint32_t*>(dst);
            if (OC == 4) {
                const uint4 v = rgb4_to_rgba(a, bb, c);
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            } else {
                d[0] = a; d[1] = bb; d[2] = c;
            }
        }
        return;
    }
    // the row's last, partial group (and every pixel of the byte form)
    for (int x = x0; x < x0 + PX && x < cv.width; x++, src += 3, dst += OC) {
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
        if (OC == 4) dst[3] = 255;
    }
}

template <int PX>
hipError_t launch_canvas_form(const RenderCanvas& cv, hipStream_t s) {
    const int groups = (cv.width + PX - 1) / PX;
    const long units = static_cast<long>(groups) * cv.height;
    const dim3 grid(static_cast<unsigned>((units + 255) / 256), static_cast<unsigned>(cv.batch));
    if (cv.channels == 4) return launch_kernel(render_canvas_kernel<PX, 4>, grid, dim3(256), 0, s, cv, groups);
    return launch_kernel(render_canvas_kernel<PX, 3>, grid, dim3(256), 0, s, cv, groups);
}

// ------------------------------------------------------------------------------------------------------------ draw phase
// Rust `as` casts from f64: truncation toward zero, saturation, NaN -> 0
__device__ __forceinline__ int as_i32(double v) {
    if (!(v == v)) return 0;
    if (v <= -2147483648.0) return -2147483647 - 1;
    if (v >= 2147483647.0) return 2147483647;
    return static_cast<int>(v);
}
__device__ __forceinline__ uint32_t as_u32(double v) {
    if (!(v > 0.0)) return 0u;  // NaN, zero and everything negative
    if (v >= 4294967295.0) return 4294967295u;
    return static_cast<uint32_t>(v);
}

struct Frame {          // one frame's canvas, as the draw phase sees it
    uint8_t* img;
    int width, height, stride, channels;
    bool dwords;        // RGBA pixels are 4-byte aligned: one dword store per pixel
};

__device__ __forceinline__ uint32_t pack(mi_color c) {
    return static_cast<uint32_t>(c.r) | (static_cast<uint32_t>(c.g) << 8) | (static_cast<uint32_t>(c.b) << 16) | (static_cast<uint32_t>(c.a) << 24);
}

// (x, y) is inside the canvas: the callers check
__device__ __forceinline__ void put(const Frame& f, int x, int y, uint32_t col) {
    uint8_t* p = f.img + static_cast<long>(y) * f.stride + static_cast<long>(f.channels) * x;
    if (f.dwords) {
        *reinterpret_cast<uint32_t*>(p) = col;
        return;
    }
    p[0] = static_cast<uint8_t>(col);
    p[1] = static_cast<uint8_t>(col >> 8);
    p[2] = static_cast<uint8_t>(col >> 16);
    if (f.channels == 4) p[3] = static_cast<uint8_t>(col >> 24);
}

// draw_filled_rect_mut(Rect::at(left, top).of_size(w, h)): the intersection with the canvas, spread over `lanes` lanes
__device__ void fill_rect(const Frame& f, long left, long top, long w, long h, uint32_t col, int lane, int lanes) {
    const long lx0 = left > 0 ? left : 0, ly0 = top > 0 ? top : 0;
    const long lx1 = left + w < f.width ? left + w : f.width, ly1 = top + h < f.height ? top + h : f.height;
    if (lx1 <= lx0 || ly1 <= ly0) return;
    const int x0 = static_cast<int>(lx0), y0 = static_cast<int>(ly0), x1 = static_cast<int>(lx1), y1 = static_cast<int>(ly1);
    const int cw = x1 - x0;
    if (cw >= lanes) {
        for (int y = y0; y < y1; y++)
            for (int x = x0 + lane; x < x1; x += lanes) put(f, x, y, col);
    } else {
        const int rows = lanes / cw, ly = lane / cw, lx = lane - ly * cw;  // `rows` rows of the rectangle per pass
        if (ly < rows)
            for (int y = y0 + ly; y < y1; y += rows) put(f, x0 + lx, y, col);
    }
}

// draw_line_segment_mut(start, end) on integer end points (render.rs:435-444: `as i32`, then `as f32`), one lane.
// Returns 1 when the line is not drawn (an end point beyond kRenderCoordLimit).
__device__ int draw_line(const Frame& f, int xs, int ys, int xe, int ye, uint32_t col) {
    const int L = kRenderCoordLimit;
    if (xs < -L || xs > L || ys < -L || ys > L || xe < -L || xe > L || ye < -L || ye > L) return 1;
    int x0 = xs, y0 = ys, x1 = xe, y1 = ye;
    const bool steep = abs(y1 - y0) > abs(x1 - x0);
    if (steep) {
        int t = x0; x0 = y0; y0 = t;
        t = x1; x1 = y1; y1 = t;
    }
    if (x0 > x1) {
        int t = x0; x0 = x1; x1 = t;
        t = y0; y0 = y1; y1 = t;
    }
    const long dx = x1 - x0, dy = abs(y1 - y0);
    const int step = y0 < y1 ? 1 : -1;
    const int major = steep ? f.height : f.width, minor = steep ? f.width : f.height;  // canvas extent along the walk / across it
    const int xa = x0 > 0 ? x0 : 0, xb = x1 < major - 1 ? x1 : major - 1;
    if (xa > xb) return 0;
    long E = dx;  // 2 * error
    int y = y0;
    if (xa > x0) {  // (dx > 0 here) the k steps in front of the canvas, in closed form
        const long k = xa - x0, T = dx - 2 * dy * k, D = 2 * dx;
        const long q = T >= 0 ? T / D : -((-T + D - 1) / D);  // floor(T / D)
        E = T - q * D;
        y = y0 - step * static_cast<int>(q);
    }
    for (int x = xa; x <= xb; x++) {
        if (y >= 0 && y < minor) {
            if (steep) put(f, y, x, col);
            else put(f, x, y, col);
        } else if (step > 0 ? y >= minor : y < 0) {
            break;  // the minor coordinate only moves away from the canvas from here on
        }
        E -= 2 * dy;
        if (E < 0) {
            y += step;
            E += 2 * dx;
        }
    }
    return 0;
}

struct P2 { double x, y; };
struct P4 { double a, b, c, d; };

// render.rs:423-433.  get(i) -> the point in pixels (f64, already scaled)
template <class Get>
__device__ void draw_points(const Frame& f, int n, double thickness, uint32_t col, Get get) {
    const uint32_t half = max(as_u32(thickness) / 2u, 1u);
    const long side = 2L * half;
    // lanes per square: its area rounded up to a power of two, at most the workgroup
    int lanes = kDrawThreads;
    if (side < 16) {
        lanes = 4;
        while (lanes < side * side) lanes *= 2;
    }
    const int group = threadIdx.x / lanes, lane = threadIdx.x % lanes, groups = kDrawThreads / lanes;
    for (int i = group; i < n; i += groups) {
        const P2 p = get(i);
        const uint32_t x = as_u32(p.x), y = as_u32(p.y);
        // `(x - w) as i32` on u32: wraps below zero
        fill_rect(f, static_cast<int>(x - half), static_cast<int>(y - half), side, side, col, lane, lanes);
    }
}

// render.rs:434-445.  get(i) -> (x_start, y_start, x_end, y_end) in pixels (f64)
template <class Get>
__device__ int draw_lines(const Frame& f, int n, uint32_t col, Get get) {
    int skipped = 0;
    for (int i = threadIdx.x; i < n; i += kDrawThreads) {
        const P4 l = get(i);
        skipped += draw_line(f, as_i32(l.a), as_i32(l.b), as_i32(l.c), as_i32(l.d), col);
    }
    return skipped;
}

// render.rs:446-462 (hollow, one lane per segment) and 463-473 (filled, one wave per rectangle).  get(i) -> (left, top, right, bottom)
template <class Get>
__device__ int draw_rects(const Frame& f, int n, bool filled, uint32_t col, Get get) {
    int skipped = 0;
    const int lanes = filled ? 64 : 1, per_item = filled ? 1 : 4;
    const long units = static_cast<long>(n) * per_item;
    const int group = threadIdx.x / lanes, lane = threadIdx.x % lanes, groups = kDrawThreads / lanes;
    for (long u = group; u < units; u += groups) {
        const int i = static_cast<int>(u / per_item), seg = static_cast<int>(u % per_item);
        const P4 r = get(i);
        const long left = as_i32(r.a), top = as_i32(r.b);
        const long w = as_u32(r.c - r.a), h = as_u32(r.d - r.b);
        const bool first = lane == 0 && seg == 0;  // the lane that counts this rectangle
        if (w == 0 || h == 0) {
            skipped += first;
            continue;
        }
        if (filled) {
            fill_rect(f, left, top, w, h, col, lane, lanes);
            continue;
        }
        const long right = left + w - 1, bottom = top + h - 1;
        const long L = kRenderCoordLimit;
        if (left < -L || left > L || top < -L || top > L || right < -L || right > L || bottom < -L || bottom > L) {
            skipped += first;
            continue;
        }
        const int l = static_cast<int>(left), t = static_cast<int>(top), rr = static_cast<int>(right), b = static_cast<int>(bottom);
        if (seg == 0) draw_line(f, l, t, rr, t, col);
        else if (seg == 1) draw_line(f, l, b, rr, b, col);
        else if (seg == 2) draw_line(f, l, t, l, b, col);
        else draw_line(f, rr, t, rr, b, col);
    }
    return skipped;
}

// What separates two annotations: every pixel of the earlier one is written before any pixel of the later one.  A frame belongs to
// one workgroup, so the fence is workgroup-scoped (a device-scoped one would add cache maintenance per annotation and order nothing more).
__device__ __forceinline__ void next_annotation() {
    __threadfence_block();
    __syncthreads();
}

__device__ __forceinline__ Frame frame_of(const RenderCanvas& cv, int b) {
    Frame f;
    f.img = cv.out + static_cast<long>(b) * cv.height * cv.out_stride;
    f.width = cv.width; f.height = cv.height; f.stride = cv.out_stride; f.channels = cv.channels;
    f.dwords = cv.channels == 4 && (reinterpret_cast<uintptr_t>(cv.out) & 3) == 0 && (cv.out_stride & 3) == 0;
    return f;
}

__device__ void store_skipped(int* skipped, int b, int mine) {
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0 && skipped) skipped[b] = total;
}

__global__ __launch_bounds__(kDrawThreads) void render_annotations_kernel(RenderCanvas cv, const mi_annotation* anns, int n_anns,
                                                                          const double* coords, long coords_per_frame, int* skipped) {
    const int b = blockIdx.x;
    const Frame f = frame_of(cv, b);
    const double* c = coords + static_cast<long>(b) * coords_per_frame;
    int mine = 0;
    for (int a = 0; a < n_anns; a++) {
        const mi_annotation A = anns[a];
        // render.rs:368-406: normalised positions times (width, height) in f64; x * 1.0 is x for every x
        const double sx = A.normalized ? static_cast<double>(cv.width) : 1.0, sy = A.normalized ? static_cast<double>(cv.height) : 1.0;
        const double* p = c + A.first;
        const uint32_t col = pack(A.color);
        auto four = [=](int i) { return P4{p[4L * i] * sx, p[4L * i + 1] * sy, p[4L * i + 2] * sx, p[4L * i + 3] * sy}; };
        if (A.kind == MI_ANN_POINTS) draw_points(f, A.count, A.thickness, col, [=](int i) { return P2{p[2L * i] * sx, p[2L * i + 1] * sy}; });
        else if (A.kind == MI_ANN_LINES) mine += draw_lines(f, A.count, col, four);
        else mine += draw_rects(f, A.count, A.kind == MI_ANN_FILLED_RECTS, col, four);
        next_annotation();
    }
    store_skipped(skipped, b, mine);
}

// detections_to_render_data (render.rs:262-313) for the n faces at `d`: the bounds annotation, then the keypoints annotation.  (sx, sy) = the
// canvas size.  Returns what was not drawn.
__device__ __forceinline__ int detection_groups(const Frame& f, const mi_detection* d, int n, double sx, double sy, const mi_render_style& st) {
    int mine = 0;
    if (st.draw_bounds && st.line_width > 0) {
        // Detection::bbox (types.rs:219-225): data[0] = (xmin, ymin), data[1] = (xmax, ymax), widened to f64
        mine += draw_rects(f, n, false, pack(st.bounds_color), [=](int i) {
            const float* v = d[i].data;
            return P4{static_cast<double>(v[0]) * sx, static_cast<double>(v[1]) * sy, static_cast<double>(v[2]) * sx, static_cast<double>(v[3]) * sy};
        });
        next_annotation();
    }
    if (st.draw_keypoints && st.point_width > 0) {
        draw_points(f, 8 * n, static_cast<double>(st.point_width), pack(st.keypoint_color), [=](int i) {
            const float* v = d[i >> 3].data + 2 * (i & 7);  // every row of `data`, the box corners included (render.rs:289-299)
            return P2{static_cast<double>(v[0]) * sx, static_cast<double>(v[1]) * sy};
        });
        next_annotation();
    }
    return mine;
}

// landmarks_to_render_data (render.rs:315-359) over rows of (x, y, z) f32: the lines annotation, then the points annotation; thickness f32 -> f64.
// What was not drawn is added to `mine`.
__device__ __forceinline__ void landmark_group(const Frame& f, double sx, double sy, int& mine, const float* lm, int n_points, int n_lines, bool face,
                                               double thickness, mi_color line_color, mi_color point_color) {
    mine += draw_lines(f, n_lines, pack(line_color), [=](int i) {
        const int s = face ? kFaceConnections[i][0] : kEyeConnections[i][0], e = face ? kFaceConnections[i][1] : kEyeConnections[i][1];
        return P4{static_cast<double>(lm[3 * s]) * sx, static_cast<double>(lm[3 * s + 1]) * sy, static_cast<double>(lm[3 * e]) * sx,
                  static_cast<double>(lm[3 * e + 1]) * sy};
    });
    next_annotation();
    draw_points(f, n_points, thickness, pack(point_color),
                [=](int i) { return P2{static_cast<double>(lm[3 * i]) * sx, static_cast<double>(lm[3 * i + 1]) * sy}; });
    next_annotation();
}

__global__ __launch_bounds__(kDrawThreads) void render_faces_kernel(RenderCanvas cv, const mi_detection* faces, const int* face_counts,
                                                                    int faces_per_frame, const float* landmarks, const int* present,
                                                                    const float* eyes, mi_render_style st, int* skipped) {
    const int b = blockIdx.x;
    const Frame f = frame_of(cv, b);
    const double sx = cv.width, sy = cv.height;
    int mine = 0;
    if (faces) {
        int n = face_counts[b];
        n = n < 0 ? 0 : (n > faces_per_frame ? faces_per_frame : n);
        mine += detection_groups(f, faces + static_cast<long>(b) * faces_per_frame, n, sx, sy, st);
    }
    const bool there = present ? present[b] != 0 : true;
    if (landmarks && st.draw_mesh && there)  // face_landmark.rs:324-339
        landmark_group(f, sx, sy, mine, landmarks + static_cast<long>(b) * MI_NUM_FACE_LANDMARKS * 3, MI_NUM_FACE_LANDMARKS, kFaceConnectionCount, true,
                       static_cast<double>(st.mesh_thickness), st.mesh_connection_color, st.mesh_landmark_color);
    if (eyes && st.draw_eyes && there)       // iris_landmark.rs:312-331, left eye then right eye
        for (int e = 0; e < 2; e++)
            landmark_group(f, sx, sy, mine, eyes + (static_cast<long>(b) * 2 + e) * kEyeRows * 3, kEyeContourPoints, kEyeConnectionCount, false,
                           static_cast<double>(st.eye_thickness), st.eye_connection_color, st.eye_landmark_color);
    store_skipped(skipped, b, mine);
}

// iris_landmarks_to_render_data (iris_landmark.rs:330-377) for one eye; iris = rows 71..75 of the eye, [5][3] f32 (IrisIndex: Center 0, Left 1,
// Top 2, Right 3, Bottom 4).  The oval annotation, then the points annotation, both of thickness `st.iris_thickness`.
__device__ __forceinline__ int iris_groups(const Frame& f, double W, double H, const float* iris, const mi_render_items_style& st) {
    int mine = 0;
    if (st.draw_iris_oval) {
        mine += draw_rects(f, 1, false, pack(st.iris_oval_color), [=](int) {
            // get_iris_diameter (iris_landmark.rs:401-418): both end points are scaled before they are subtracted
            auto dist = [=](int a, int b) {
                const double x0 = static_cast<double>(iris[3 * a]) * W, y0 = static_cast<double>(iris[3 * a + 1]) * H;
                const double x1 = static_cast<double>(iris[3 * b]) * W, y1 = static_cast<double>(iris[3 * b + 1]) * H;
                return __dsqrt_rn((x0 - x1) * (x0 - x1) + (y0 - y1) * (y0 - y1));
            };
            const double radius = (dist(2, 4) + dist(1, 3)) / 2.0 / 2.0;  // (vert + horiz) / 2. (:417), then / 2.0 (:340)
            // :345-346 divide by the size, render.rs:368-406 multiplies by it again: two roundings, kept
            const double radius_h = radius / W, radius_v = radius / H;
            const double cx = static_cast<double>(iris[0]), cy = static_cast<double>(iris[1]);
            return P4{(cx - radius_h) * W, (cy - radius_v) * H, (cx + radius_h) * W, (cy + radius_v) * H};
        });
        next_annotation();
    }
    if (st.draw_iris_points) {
        draw_points(f, MI_NUM_IRIS_LANDMARKS, st.iris_thickness, pack(st.iris_landmark_color),
                    [=](int i) { return P2{static_cast<double>(iris[3 * i]) * W, static_cast<double>(iris[3 * i + 1]) * H}; });
        next_annotation();
    }
    return mine;
}

// first slot of item_frame[0, used) whose frame is not below b.  item_frame is only compared: whatever it holds, the result is in [0, used]
__device__ __forceinline__ int first_slot_of(const int* item_frame, int used, int b) {
    int lo = 0, hi = used;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (item_frame[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The draw phase of mi_render_face_items: the frame's detections, then every item of the frame in slot order.  Everything that decides whether
// an annotation is drawn (the slot range, present, the style) is the same for all lanes of the workgroup, as next_annotation() needs.
__global__ __launch_bounds__(kDrawThreads) void render_face_items_kernel(RenderCanvas cv, const mi_detection* faces, const int* face_counts,
                                                                         int max_faces, const int* item_frame, const int* n_items, int max_items,
                                                                         const float* landmarks, const int* present, const float* eyes,
                                                                         mi_render_items_style st, int* skipped) {
    const int b = blockIdx.x;
    const Frame f = frame_of(cv, b);
    const double sx = cv.width, sy = cv.height;
    int mine = 0;
    if (faces) {
        int n = face_counts[b];
        n = n < 0 ? 0 : (n > max_faces ? max_faces : n);
        mine += detection_groups(f, faces + static_cast<long>(b) * max_faces, n, sx, sy, st.base);
    }
    if (item_frame) {
        int used = n_items[0];
        used = used < 0 ? 0 : (used > max_items ? max_items : used);
        const int first = first_slot_of(item_frame, used, b), last = first_slot_of(item_frame, used, b + 1);
        for (int j = first; j < last; j++) {
            // (a list out of order: a slot of another frame inside the range is left out)
            const bool there = item_frame[j] == b && (present ? present[j] != 0 : true);
            if (!there) continue;
            const mi_render_style& base = st.base;
            if (landmarks && base.draw_mesh)  // face_landmark.rs:324-339
                landmark_group(f, sx, sy, mine, landmarks + static_cast<long>(j) * MI_NUM_FACE_LANDMARKS * 3, MI_NUM_FACE_LANDMARKS, kFaceConnectionCount,
                               true, static_cast<double>(base.mesh_thickness), base.mesh_connection_color, base.mesh_landmark_color);
            if (!eyes) continue;
            const float* eye = eyes + static_cast<long>(j) * 2 * kEyeRows * 3;
            if (base.draw_eyes)               // iris_landmark.rs:312-331, left eye then right eye
                for (int e = 0; e < 2; e++)
                    landmark_group(f, sx, sy, mine, eye + e * kEyeRows * 3, kEyeContourPoints, kEyeConnectionCount, false,
                                   static_cast<double>(base.eye_thickness), base.eye_connection_color, base.eye_landmark_color);
            for (int e = 0; e < 2; e++)       // iris_landmark.rs:330-377, left iris then right iris
                mine += iris_groups(f, sx, sy, eye + (e * kEyeRows + MI_NUM_EYE_LANDMARKS) * 3, st);
        }
    }
    store_skipped(skipped, b, mine);
}

inline bool aligned_to(const void* p, long stride, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0 && stride % n == 0; }

}  // namespace

hipError_t launch_render_canvas(const RenderCanvas& cv, hipStream_t s) {
    if (cv.out == cv.frames) return hipSuccess;  // in place
    if (aligned_to(cv.frames, cv.stride, 16) && aligned_to(cv.out, cv.out_stride, 16)) return launch_canvas_form<16>(cv, s);
    if (aligned_to(cv.frames, cv.stride, 4) && aligned_to(cv.out, cv.out_stride, 4)) return launch_canvas_form<4>(cv, s);
    return launch_canvas_form<1>(cv, s);
}

hipError_t launch_render_annotations(const RenderCanvas& cv, const mi_annotation* d_anns, int n_anns, const double* d_coords,
                                     long coords_per_frame, int* d_skipped, hipStream_t s) {
    return launch_kernel(render_annotations_kernel, dim3(cv.batch), dim3(kDrawThreads), 0, s, cv, d_anns, n_anns, d_coords, coords_per_frame, d_skipped);
}

hipError_t launch_render_faces(const RenderCanvas& cv, const mi_detection* d_faces, const int* d_face_counts, int faces_per_frame,
                               const float* d_landmarks, const int* d_present, const float* d_eyes, const mi_render_style& style,
                               int* d_skipped, hipStream_t s) {
    return launch_kernel(render_faces_kernel, dim3(cv.batch), dim3(kDrawThreads), 0, s, cv, d_faces, d_face_counts, faces_per_frame, d_landmarks,
                         d_present, d_eyes, style, d_skipped);
}

hipError_t launch_render_face_items(const RenderCanvas& cv, const mi_detection* d_faces, const int* d_face_counts, int max_faces,
                                    const int* d_item_frame, const int* d_n_items, int max_items, const float* d_landmarks, const int* d_present,
                                    const float* d_eyes, const mi_render_items_style& style, int* d_skipped, hipStream_t s) {
    return launch_kernel(render_face_items_kernel, dim3(cv.batch), dim3(kDrawThreads), 0, s, cv, d_faces, d_face_counts, max_faces, d_item_frame,
                         d_n_items, max_items, d_landmarks, d_present, d_eyes, style, d_skipped);
}

}  // namespace mi
