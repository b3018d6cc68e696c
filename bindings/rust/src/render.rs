//! The reference's `render.rs` by name — **source only, never compiled** (no Rust toolchain where this repository is built):
//! `Color`, `Colors`, the annotation types, `detections_to_render_data`, `landmarks_to_render_data` and `render_to_image`,
//! plus `face_landmarks_to_render_data` / `eye_landmarks_to_render_data` (face_landmark.rs:324-339, iris_landmark.rs:312-331).
//!
//! The builders are plain data shuffling and stay on the host, as in the reference.  `render_to_image` draws on the GPU through
//! `mi_render_annotations` (include/mi_face.h, "render.rs"): the items of every annotation are flattened, in order, into runs of
//! one kind and one colour — a `FilledRectOrOval` carries its own fill colour (render.rs:466), so a run ends where the fill
//! changes — which keeps the reference's drawing order item for item.  Deviations from the reference (both reported by the C
//! entry's `skipped` count, returned here next to the picture): empty rectangles are not drawn instead of panicking, and lines
//! with an end point beyond 2^20 px are not drawn instead of being walked for up to 2^32 steps.
//! A caller whose results are already in device memory uses `ffi::mi_render_faces` and never builds annotations at all;
//! `render_face_items` draws the item list of `mi_pipeline_run_faces` (every face of a frame, both irises included) the same way
//! from host memory, and `iris_landmarks_to_render_data` (iris_landmark.rs:330-377) is the host builder of the iris annotations.
use crate::ffi;
use crate::types::{Detection, Image, Landmark};
use anyhow::Error;

/// render.rs:6-12
#[derive(Debug, Clone, Copy)]
pub struct Color {
    pub r: i32,
    pub g: i32,
    pub b: i32,
    pub a: Option<i32>,
}

impl Color {
    pub fn new(r: Option<i32>, g: Option<i32>, b: Option<i32>, a: Option<i32>) -> Self {
        Self { r: r.unwrap_or(0), g: g.unwrap_or(0), b: b.unwrap_or(0), a }
    }

    pub fn as_tuple(&self) -> (i32, i32, i32, Option<i32>) {
        (self.r, self.g, self.b, self.a)
    }

    /// the four bytes render_to_image writes (render.rs:431)
    pub(crate) fn to_mi(self) -> ffi::mi_color {
        ffi::mi_color { r: self.r as u8, g: self.g as u8, b: self.b as u8, a: self.a.unwrap_or(255) as u8 }
    }
}

/// render.rs:28-68
#[derive(Debug, Clone, Copy)]
pub struct Colors;

impl Colors {
    pub const BLACK: Color = Color { r: 0, g: 0, b: 0, a: None };
    pub const RED: Color = Color { r: 255, g: 0, b: 0, a: None };
    pub const GREEN: Color = Color { r: 0, g: 255, b: 0, a: None };
    pub const BLUE: Color = Color { r: 0, g: 0, b: 255, a: None };
    pub const PINK: Color = Color { r: 255, g: 0, b: 255, a: None };
    pub const WHITE: Color = Color { r: 255, g: 255, b: 255, a: None };
}

/// render.rs:70-92
#[derive(Debug, Clone, Copy)]
pub struct Point {
    pub x: f64,
    pub y: f64,
}

impl Point {
    pub fn new(x: f64, y: f64) -> Self {
        Self { x, y }
    }
}

/// render.rs:94-128 (`oval` is carried and, as in the reference, draws the same rectangle)
#[derive(Debug, Clone, Copy)]
pub struct RectOrOval {
    pub left: f64,
    pub top: f64,
    pub right: f64,
    pub bottom: f64,
    pub oval: bool,
}

impl RectOrOval {
    pub fn new(left: f64, top: f64, right: f64, bottom: f64, oval: bool) -> Self {
        Self { left, top, right, bottom, oval }
    }
}

/// render.rs:130-147
#[derive(Debug, Clone, Copy)]
pub struct FilledRectOrOval {
    pub rect: RectOrOval,
    pub fill: Color,
}

/// render.rs:149-184 (`dashed` is carried and ignored, as in the reference)
#[derive(Debug, Clone, Copy)]
pub struct Line {
    pub x_start: f64,
    pub y_start: f64,
    pub x_end: f64,
    pub y_end: f64,
    pub dashed: bool,
}

impl Line {
    pub fn new(x_start: f64, y_start: f64, x_end: f64, y_end: f64, dashed: bool) -> Self {
        Self { x_start, y_start, x_end, y_end, dashed }
    }
}

/// render.rs:186-192
#[derive(Debug, Clone, Copy)]
pub enum AnnotationData {
    Point(Point),
    RectOrOval(RectOrOval),
    FilledRectOrOval(FilledRectOrOval),
    Line(Line),
}

/// render.rs:207-213
#[derive(Debug, Clone)]
pub struct Annotation {
    pub data: Vec<AnnotationData>,
    pub normalized_positions: bool,
    pub thickness: f64,
    pub color: Color,
}

impl Annotation {
    pub fn new(data: Vec<AnnotationData>, normalized_positions: bool, thickness: f64, color: Color) -> Self {
        Self { data, normalized_positions, thickness, color }
    }
}

/// render.rs:262-313
pub fn detections_to_render_data(
    detections: Vec<Detection>, bounds_color: Option<Color>, keypoint_color: Option<Color>, line_width: i32, point_width: i32,
    normalized_positions: bool, output: Option<Vec<Annotation>>,
) -> Vec<Annotation> {
    let mut out = output.unwrap_or_default();
    if let Some(color) = bounds_color {
        if line_width > 0 {
            let data = detections
                .iter()
                .map(|d| {
                    let b = d.bbox();
                    AnnotationData::RectOrOval(RectOrOval::new(b.xmin, b.ymin, b.xmax, b.ymax, false))
                })
                .collect();
            out.push(Annotation::new(data, normalized_positions, line_width as f64, color));
        }
    }
    if let Some(color) = keypoint_color {
        if point_width > 0 {
            // every row of `data`, the two box corners included (render.rs:289-299)
            let data = detections
                .iter()
                .flat_map(|d| d.data.iter().map(|row| AnnotationData::Point(Point::new(row[0] as f64, row[1] as f64))).collect::<Vec<_>>())
                .collect();
            out.push(Annotation::new(data, normalized_positions, point_width as f64, color));
        }
    }
    out
}

/// render.rs:315-359: the lines annotation, then the points annotation
pub fn landmarks_to_render_data(
    landmarks: Vec<Landmark>, landmark_connections: Vec<(i32, i32)>, landmark_color: Option<Color>, connection_color: Option<Color>,
    thickness: Option<f32>, normalized_positions: Option<bool>, output: Option<Vec<Annotation>>,
) -> Vec<Annotation> {
    let thickness = thickness.unwrap_or(1.) as f64;
    let normalized = normalized_positions.unwrap_or(true);
    let lines = landmark_connections
        .iter()
        .map(|&(s, e)| {
            let (a, b) = (&landmarks[s as usize], &landmarks[e as usize]);
            AnnotationData::Line(Line::new(a.x, a.y, b.x, b.y, false))
        })
        .collect();
    let points = landmarks.iter().map(|l| AnnotationData::Point(Point::new(l.x, l.y))).collect();
    let mut out = output.unwrap_or_default();
    out.push(Annotation::new(lines, normalized, thickness, connection_color.unwrap_or(Colors::RED)));
    out.push(Annotation::new(points, normalized, thickness, landmark_color.unwrap_or(Colors::RED)));
    out
}

/// face_landmark.rs:35-166, as chains: consecutive entries of a chain are connected (124 connections)
const FACE_CHAINS: [&[i32]; 13] = [
    &[61, 146, 91, 181, 84, 17, 314, 405, 321, 375, 291],
    &[61, 185, 40, 39, 37, 0, 267, 269, 270, 409, 291],
    &[78, 95, 88, 178, 87, 14, 317, 402, 318, 324, 308],
    &[78, 191, 80, 81, 82, 13, 312, 311, 310, 415, 308],
    &[33, 7, 163, 144, 145, 153, 154, 155, 133],
    &[33, 246, 161, 160, 159, 158, 157, 173, 133],
    &[46, 53, 52, 65, 55],
    &[70, 63, 105, 66, 107],
    &[263, 249, 390, 373, 374, 380, 381, 382, 362],
    &[263, 466, 388, 387, 386, 385, 384, 398, 362],
    &[276, 283, 282, 295, 285],
    &[300, 293, 334, 296, 336],
    &[10, 338, 297, 332, 284, 251, 389, 356, 454, 323, 361, 288, 397, 365, 379, 378, 400, 377, 152, 148, 176, 149, 150, 136, 172, 58, 132,
      93, 234, 127, 162, 21, 54, 103, 67, 109, 10],
];

/// FACE_LANDMARK_CONNECTIONS — face_landmark.rs:35-166
pub fn face_landmark_connections() -> Vec<(i32, i32)> {
    FACE_CHAINS.iter().flat_map(|c| c.windows(2).map(|w| (w[0], w[1])).collect::<Vec<_>>()).collect()
}

/// EYE_LANDMARK_CONNECTIONS — iris_landmark.rs:44-60; MAX_EYE_LANDMARK = 15 (iris_landmark.rs:62)
pub fn eye_landmark_connections() -> Vec<(i32, i32)> {
    let mut v: Vec<(i32, i32)> = (0..8).map(|i| (i, i + 1)).collect();
    v.extend((9..14).map(|i| (i, i + 1)));
    v.push((0, 9));
    v.push((8, 14));
    v
}

/// face_landmark.rs:324-339
pub fn face_landmarks_to_render_data(
    face_landmarks: Vec<Landmark>, landmark_color: Color, connection_color: Color, thickness: Option<f32>, output: Option<Vec<Annotation>>,
) -> Vec<Annotation> {
    landmarks_to_render_data(face_landmarks, face_landmark_connections(), Some(landmark_color), Some(connection_color), thickness, None, output)
}

/// iris_landmark.rs:312-331: the first 15 contour points and their 15 connections
pub fn eye_landmarks_to_render_data(
    eye_contour: Vec<Landmark>, landmark_color: Color, connection_color: Color, thickness: Option<f32>, output: Option<Vec<Annotation>>,
) -> Vec<Annotation> {
    let n = eye_landmark_connections().len().min(eye_contour.len());
    landmarks_to_render_data(eye_contour[..n].to_vec(), eye_landmark_connections(), Some(landmark_color), Some(connection_color), thickness, None, output)
}

/// What `render_to_image` returns where the reference returns a `DynamicImage::ImageRgba8`: RGBA rows of `4 * width` bytes.
#[derive(Debug, Clone)]
pub struct RgbaImage {
    pub data: Vec<u8>,
    pub width: i32,
    pub height: i32,
    /// items the C ABI did not draw (empty rectangles, lines beyond 2^20 px)
    pub skipped: i32,
}

/// render.rs:361-479 on device 0 (`blend_mode` is read and never used, as in the reference)
pub fn render_to_image<'a, I>(annotations: &Vec<Annotation>, image: I, blend_mode: Option<bool>) -> Result<RgbaImage, Error>
where
    I: TryInto<Image<'a>>,
    I::Error: Into<Error>,
{
    let _blend = blend_mode.unwrap_or(false);
    let image: Image<'a> = image.try_into().map_err(Into::into)?;
    let mut anns: Vec<ffi::mi_annotation> = Vec::new();
    let mut coords: Vec<f64> = Vec::new();
    for annotation in annotations {
        for item in &annotation.data {
            let (kind, color, values): (i32, Color, Vec<f64>) = match item {
                AnnotationData::Point(p) => (ffi::MI_ANN_POINTS, annotation.color, vec![p.x, p.y]),
                AnnotationData::Line(l) => (ffi::MI_ANN_LINES, annotation.color, vec![l.x_start, l.y_start, l.x_end, l.y_end]),
                AnnotationData::RectOrOval(r) => (ffi::MI_ANN_RECTS, annotation.color, vec![r.left, r.top, r.right, r.bottom]),
                AnnotationData::FilledRectOrOval(f) => {
                    (ffi::MI_ANN_FILLED_RECTS, f.fill, vec![f.rect.left, f.rect.top, f.rect.right, f.rect.bottom])
                }
            };
            let color = color.to_mi();
            let normalized = annotation.normalized_positions as i32;
            let same_run = match anns.last() {
                Some(a) => a.kind == kind && a.color == color && a.normalized == normalized && a.thickness.to_bits() == annotation.thickness.to_bits(),
                None => false,
            };
            if same_run {
                anns.last_mut().unwrap().count += 1;
            } else {
                anns.push(ffi::mi_annotation { kind, first: coords.len() as i32, count: 1, thickness: annotation.thickness, color, normalized });
            }
            coords.extend(values);
        }
    }
    let (w, h) = (image.width(), image.height());
    let mut out = vec![0u8; 4 * w as usize * h as usize];
    let mut skipped = 0i32;
    crate::check(unsafe {
        ffi::mi_render_annotations(
            0, image.data().as_ptr(), 1, w, h, image.stride(), anns.as_ptr(), anns.len() as i32, coords.as_ptr(), coords.len() as _,
            out.as_mut_ptr(), 4, 4 * w, &mut skipped, ffi::MI_MEM_HOST, std::ptr::null_mut(),
        )
    })?;
    Ok(RgbaImage { data: out, width: w, height: h, skipped })
}

/// iris_landmark.rs:330-377: the oval annotation (when `oval_color` is given; needs an image of at least 2 x 2), then the points
/// annotation (when `landmark_color` is given), both normalised and of `thickness` (1.0 when None).
pub fn iris_landmarks_to_render_data(
    iris_landmarks: Vec<Landmark>, landmark_color: Option<Color>, oval_color: Option<Color>, thickness: Option<f64>,
    image_size: Option<(i32, i32)>, output: Option<Vec<Annotation>>,
) -> Result<Vec<Annotation>, Error> {
    let thickness = thickness.unwrap_or(1.0);
    let (w, h) = image_size.unwrap_or((-1, -1));
    let mut out = output.unwrap_or_default();
    if let Some(color) = oval_color {
        if w < 2 || h < 2 {
            return Err(Error::msg("oval_color requires a valid image_size arg"));
        }
        let (wf, hf) = (w as f64, h as f64);
        // IrisIndex: Center 0, Left 1, Top 2, Right 3, Bottom 4; get_iris_diameter (iris_landmark.rs:401-418) in pixels
        let span = |a: usize, b: usize| -> f64 {
            let (p, q) = (&iris_landmarks[a], &iris_landmarks[b]);
            let (dx, dy) = (p.x * wf - q.x * wf, p.y * hf - q.y * hf);
            (dx * dx + dy * dy).sqrt()
        };
        let radius = (span(2, 4) + span(1, 3)) / 2. / 2.0;
        let (rh, rv) = (radius / wf, radius / hf);
        let c = &iris_landmarks[0];
        let oval = RectOrOval::new(c.x - rh, c.y - rv, c.x + rh, c.y + rv, true);
        out.push(Annotation::new(vec![AnnotationData::RectOrOval(oval)], true, thickness, color));
    }
    if let Some(color) = landmark_color {
        let points = iris_landmarks.iter().map(|l| AnnotationData::Point(Point::new(l.x, l.y))).collect();
        out.push(Annotation::new(points, true, thickness, color));
    }
    Ok(out)
}

/// The item list of `mi_pipeline_run_faces`, in host memory, as `render_face_items` reads it (include/mi_face.h).  Every group may be left
/// out, as the C entry allows: `faces` (with its counts and `max_faces`), the item list itself, and `landmarks`, `present`, `eyes` inside it.
pub struct FaceItems<'a> {
    /// (faces [batch][max_faces], face_counts [batch], max_faces 1..16)
    pub faces: Option<(&'a [ffi::mi_detection], &'a [i32], i32)>,
    /// (item_frame [max_items], n_items: the slots used first)
    pub items: Option<(&'a [i32], &'a [i32])>,
    /// f32 [max_items][468][3]
    pub landmarks: Option<&'a [f32]>,
    /// [max_items]; None: every used slot is drawn
    pub present: Option<&'a [i32]>,
    /// f32 [max_items][2][76][3]
    pub eyes: Option<&'a [f32]>,
}

fn ptr_or_null<T>(s: Option<&[T]>) -> *const T {
    s.map_or(std::ptr::null(), |s| s.as_ptr())
}

/// `mi_render_face_items` on device 0 for `batch` tightly packed RGB frames in host memory: boxes and key points of every frame,
/// then mesh, eyes and irises of every item of the frame.  Returns one RGBA picture per frame.
pub fn render_face_items(
    frames: &[u8], batch: i32, width: i32, height: i32, items: &FaceItems, style: &ffi::mi_render_items_style,
) -> Result<Vec<RgbaImage>, Error> {
    if batch < 1 || width < 1 || height < 1 {
        return Err(Error::msg("batch, width and height must be positive"));
    }
    let b = batch as usize;
    let frame_bytes = 3 * width as usize * height as usize;
    if frames.len() < b * frame_bytes {
        return Err(Error::msg("frames must hold batch tightly packed RGB pictures"));
    }
    let max_faces = match items.faces {
        Some((faces, counts, f)) => {
            if !(1..=16).contains(&f) || faces.len() < b * f as usize || counts.len() < b {
                return Err(Error::msg("faces need max_faces in 1..16, batch * max_faces detections and batch counts"));
            }
            f
        }
        None => 1,
    };
    // the size every per-item array must have; 1 (and unused) without an item list
    let m = match items.items {
        Some((item_frame, n_items)) => {
            if item_frame.is_empty() || item_frame.len() > 32767 || n_items.is_empty() {
                return Err(Error::msg("item_frame must hold 1..32767 slots and n_items at least the count of used slots"));
            }
            item_frame.len()
        }
        None => {
            if items.landmarks.is_some() || items.eyes.is_some() {
                return Err(Error::msg("landmarks and eyes need the item list"));
            }
            1
        }
    };
    let short = |s: Option<usize>, need: usize| s.map_or(false, |len| len < need);
    if short(items.landmarks.map(|s| s.len()), m * 468 * 3) || short(items.eyes.map(|s| s.len()), m * 2 * 76 * 3)
        || short(items.present.map(|s| s.len()), m)
    {
        return Err(Error::msg("an item array is shorter than max_items items"));
    }
    let out_bytes = 4 * width as usize * height as usize;
    let mut out = vec![0u8; b * out_bytes];
    let mut skipped = vec![0i32; b];
    crate::check(unsafe {
        ffi::mi_render_face_items(
            0, frames.as_ptr(), batch, width, height, 3 * width, ptr_or_null(items.faces.map(|f| f.0)), ptr_or_null(items.faces.map(|f| f.1)),
            max_faces, ptr_or_null(items.items.map(|i| i.0)), ptr_or_null(items.items.map(|i| i.1)), m as i32, ptr_or_null(items.landmarks),
            ptr_or_null(items.items.and(items.present)), ptr_or_null(items.eyes), style, out.as_mut_ptr(), 4, 4 * width, skipped.as_mut_ptr(),
            ffi::MI_MEM_HOST, std::ptr::null_mut(),
        )
    })?;
    Ok(out.chunks(out_bytes).zip(skipped).map(|(px, s)| RgbaImage { data: px.to_vec(), width, height, skipped: s }).collect())
}
