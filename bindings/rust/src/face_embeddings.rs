//! face_embeddings.rs:22-109 of the reference.  The MODEL IS THE CALLER'S: the reference ships no `face_embeddings.tflite` (its README
//! tells users to download one), none is shipped here, and the reference's own model has never been run on this engine.  Any graph of
//! the operators the engine lowers that maps `[1,112,112,3]` to one output of `D` values per frame loads.
use crate::pipeline::FacesResults;
use crate::types::{BBox, Detection, Image, Rect};
use crate::{check, ffi};
use anyhow::Error;
use std::ffi::CString;

/// `IMG_SIZE` — face_embeddings.rs:20
pub const IMG_SIZE: i32 = 112;

pub struct FaceEmbeddings {
    handle: *mut ffi::mi_fe,
    features: usize,
}

unsafe impl Send for FaceEmbeddings {}
unsafe impl Sync for FaceEmbeddings {}

/// What `infer_items` returns: one row per item of `Pipeline::run_faces`, zeros where `valid` is 0.
pub struct ItemEmbeddings {
    pub features: usize,
    /// `[max_items][features]`, l2-normalised
    pub embeddings: Vec<f32>,
    /// `[max_items]`: 1 = the item has an embedding (a used slot whose box lies inside its frame)
    pub valid: Vec<i32>,
    /// `[max_items][features]` when asked for: the network's output before `l2_norm`
    pub raw: Vec<f32>,
    /// `[max_items][112][112][3]` when asked for: the network's input
    pub chips: Vec<f32>,
}

impl FaceEmbeddings {
    /// `FaceEmbeddings::new(model_path)` — face_embeddings.rs:30-44.  `model_path` is the model FILE (default
    /// "./models/face_embeddings.tflite", :36).
    pub fn new(model_path: Option<String>) -> Result<FaceEmbeddings, Error> {
        Self::new_on_device(model_path, 0)
    }

    pub fn new_on_device(model_path: Option<String>, device: i32) -> Result<FaceEmbeddings, Error> {
        let path = match model_path {
            Some(p) => Some(CString::new(p)?),
            None => None,
        };
        let mut handle: *mut ffi::mi_fe = std::ptr::null_mut();
        check(unsafe { ffi::mi_fe_create(path.as_ref().map_or(std::ptr::null(), |p| p.as_ptr()), device, &mut handle) })?;
        let mut d: i32 = 0;
        let rc = unsafe { ffi::mi_fe_features(handle, &mut d) };
        if rc != ffi::MI_OK {
            unsafe { ffi::mi_fe_free(handle) };
            return Err(crate::last_error(rc));
        }
        Ok(FaceEmbeddings { handle, features: d.max(0) as usize })
    }

    /// `D`: 128 or 512 by the reference's doc comment (face_embeddings.rs:29); whatever the caller's graph produces here.
    pub fn features(&self) -> usize {
        self.features
    }

    /// Operand precision of the network's dense k x k convolutions (engine option "conv_bf16" on the handle's model): "f32" (default),
    /// "bf16" (operands rounded to bf16) or "bf16x3" (operands split into two bf16 values: about f32 accuracy).  Anything else is an `Err`.
    pub fn set_precision(&self, precision: &str) -> Result<(), Error> {
        let value = match precision {
            "f32" => 0,
            "bf16" => 1,
            "bf16x3" => 2,
            other => return Err(anyhow::anyhow!("precision must be \"f32\", \"bf16\" or \"bf16x3\", not {:?}", other)),
        };
        let key = CString::new("conv_bf16")?;
        check(unsafe { ffi::mi_model_set_option(ffi::mi_fe_model(self.handle), key.as_ptr(), value) })
    }

    pub fn precision(&self) -> Result<&'static str, Error> {
        let key = CString::new("conv_bf16")?;
        let mut value: i32 = 0;
        check(unsafe { ffi::mi_model_get_option(ffi::mi_fe_model(self.handle), key.as_ptr(), &mut value) })?;
        Ok(match value {
            1 => "bf16",
            2 => "bf16x3",
            _ => "f32",
        })
    }

    /// `infer(&self, image, bbox) -> Result<Array2<f32>>` — face_embeddings.rs:46-89, the `[1, D]` array as its row: `bbox` in absolute
    /// pixels (`faces[0].bbox().scale(size)`, :128), `crop_image_to_bbox`, `image_to_tensor(crop, None, (112, 112), false, (0, 1), false)`,
    /// the network, `l2_norm`.  Where the reference panics (`Mat::roi(..).unwrap()`, :107: a box that leaves the image) this is an `Err`.
    pub fn infer<'a, I>(&self, image: I, bbox: BBox) -> Result<Vec<f32>, Error>
    where
        I: TryInto<Image<'a>>,
        I::Error: Into<Error>,
    {
        let image: Image<'a> = image.try_into().map_err(Into::into)?;
        let b = [bbox.xmin, bbox.ymin, bbox.xmax, bbox.ymax];
        let mut out = vec![0f32; self.features];
        check(unsafe {
            ffi::mi_fe_infer_image(self.handle, image.data.as_ptr(), image.width, image.height, image.stride, b.as_ptr(), out.as_mut_ptr(),
                                   out.len() as i32)
        })?;
        Ok(out)
    }

    /// `infer` for every item of what `Pipeline::run_faces` returned for these frames (`mi_fe_infer_face_items`): chips, network and
    /// `l2_norm` on the device, one call.
    pub fn infer_items(&self, frames: &[u8], batch: usize, width: i32, height: i32, stride: i32, faces: &FacesResults, want_raw: bool,
                       want_chips: bool) -> Result<ItemEmbeddings, Error> {
        let m = faces.item_frame.len();
        // FacesResults holds the detections of a frame as a Vec of its own: back to the [batch][max_faces] block the C entry reads
        let max_faces = faces.faces.iter().map(|f| f.len()).max().unwrap_or(0).max(1);
        if batch == 0 || m == 0 || m > 32767 || faces.item_face.len() != m || faces.faces.len() != batch || max_faces > 16 {
            return Err(Error::msg("the result of run_faces on these frames is expected (max_faces 1..16, max_items 1..32767)"));
        }
        let mut dets = vec![ffi::mi_detection { data: [0.0; 16], score: 0.0 }; batch * max_faces];
        for (b, frame) in faces.faces.iter().enumerate() {
            for (k, det) in frame.iter().enumerate() {
                dets[b * max_faces + k] = det.to_mi();
            }
        }
        if width <= 0 || height <= 0 || stride <= 0 || (stride as i64) < 3 * width as i64 {
            return Err(Error::msg("frames must hold batch frames of height rows of stride bytes"));
        }
        let (w, h, s) = (width as usize, height as usize, stride as usize);
        let need = s.checked_mul(h).and_then(|f| f.checked_mul(batch - 1)).and_then(|x| x.checked_add(s * (h - 1))).and_then(|x| x.checked_add(3 * w));
        if need.map_or(true, |x| frames.len() < x) {
            return Err(Error::msg("frames must hold batch frames of height rows of stride bytes"));
        }
        let d = self.features;
        let chip = 3 * (IMG_SIZE as usize) * (IMG_SIZE as usize);
        let mut out = ItemEmbeddings {
            features: d,
            embeddings: vec![0f32; m * d],
            valid: vec![0i32; m],
            raw: vec![0f32; if want_raw { m * d } else { 0 }],
            chips: vec![0f32; if want_chips { m * chip } else { 0 }],
        };
        check(unsafe {
            ffi::mi_fe_infer_face_items(self.handle, frames.as_ptr(), batch as i32, width, height, stride, dets.as_ptr(), max_faces as i32,
                                        faces.item_frame.as_ptr(), faces.item_face.as_ptr(), m as i32,
                                        out.embeddings.as_mut_ptr(), out.valid.as_mut_ptr(),
                                        if want_raw { out.raw.as_mut_ptr() } else { std::ptr::null_mut() },
                                        if want_chips { out.chips.as_mut_ptr() } else { std::ptr::null_mut() }, ffi::MI_MEM_HOST,
                                        std::ptr::null_mut())
        })?;
        Ok(out)
    }

    /// NOT the reference's chip (that is `infer`, which crops the box): the least-squares similarity fit of `points` — pixel coordinates in
    /// the order of `face_align_template(source)`, five of them, four for `AlignSource::Detection` — the warp of the WHOLE image by it to
    /// 112 x 112, the network, `l2_norm` (`mi_fe_infer_image_aligned`).  Returns the embedding and the fitted ROI; points without a fit
    /// (a coordinate that is not finite, all points equal) are an `Err`.
    pub fn infer_aligned<'a, I>(&self, image: I, points: &[[f32; 2]], source: AlignSource) -> Result<(Vec<f32>, Rect), Error>
    where
        I: TryInto<Image<'a>>,
        I::Error: Into<Error>,
    {
        let image: Image<'a> = image.try_into().map_err(Into::into)?;
        let mut out = vec![0f32; self.features];
        let mut roi = Rect::new(0.5, 0.5, 1.0, 1.0, 0.0, true).to_mi();
        check(unsafe {
            ffi::mi_fe_infer_image_aligned(self.handle, image.data.as_ptr(), image.width, image.height, image.stride, points.as_ptr() as *const f32,
                                           points.len() as i32, source.to_mi(), out.as_mut_ptr(), out.len() as i32, &mut roi)
        })?;
        Ok((out, Rect::from_mi(&roi)))
    }

    /// `infer_aligned` for every item of what `Pipeline::run_faces` returned for these frames (`mi_fe_infer_aligned_items`): the points of
    /// an item come from its mesh (`AlignSource::Mesh`: landmarks and `present`), from its detection's key points (`AlignSource::Detection`)
    /// or from the caller (`AlignSource::Points`: `points` holds `[max_items][5]` pixel points).  `rois` holds the fitted ROI of every item.
    pub fn infer_items_aligned(&self, frames: &[u8], batch: usize, width: i32, height: i32, stride: i32, faces: &FacesResults,
                               source: AlignSource, points: Option<&[[f32; 2]]>, want_raw: bool, want_chips: bool)
                               -> Result<(ItemEmbeddings, Vec<Rect>), Error> {
        let m = faces.item_frame.len();
        let max_faces = faces.faces.iter().map(|f| f.len()).max().unwrap_or(0).max(1);
        if batch == 0 || m == 0 || m > 32767 || faces.item_face.len() != m || faces.faces.len() != batch || max_faces > 16 {
            return Err(Error::msg("the result of run_faces on these frames is expected (max_faces 1..16, max_items 1..32767)"));
        }
        if width <= 0 || height <= 0 || stride <= 0 || (stride as i64) < 3 * width as i64 {
            return Err(Error::msg("frames must hold batch frames of height rows of stride bytes"));
        }
        let (w, h, s) = (width as usize, height as usize, stride as usize);
        let need = s.checked_mul(h).and_then(|f| f.checked_mul(batch - 1)).and_then(|x| x.checked_add(s * (h - 1))).and_then(|x| x.checked_add(3 * w));
        if need.map_or(true, |x| frames.len() < x) {
            return Err(Error::msg("frames must hold batch frames of height rows of stride bytes"));
        }
        // the operand the source reads, as the C entry wants it, and its gate
        let mut dets: Vec<ffi::mi_detection> = Vec::new();
        let present: Vec<i32> = faces.present.iter().map(|&p| p as i32).collect();
        let (src, gate): (*const std::ffi::c_void, *const i32) = match source {
            AlignSource::Mesh => {
                if faces.landmarks.len() != m * 468 * 3 || present.len() != m {
                    return Err(Error::msg("landmarks must be [max_items][468][3] and present [max_items]"));
                }
                (faces.landmarks.as_ptr() as *const std::ffi::c_void, present.as_ptr())
            }
            AlignSource::Detection => {
                dets = vec![ffi::mi_detection { data: [0.0; 16], score: 0.0 }; batch * max_faces];
                for (b, frame) in faces.faces.iter().enumerate() {
                    for (k, det) in frame.iter().enumerate() {
                        dets[b * max_faces + k] = det.to_mi();
                    }
                }
                (dets.as_ptr() as *const std::ffi::c_void, std::ptr::null())
            }
            AlignSource::Points => match points {
                Some(p) if p.len() == m * 5 => (p.as_ptr() as *const std::ffi::c_void, std::ptr::null()),
                _ => return Err(Error::msg("AlignSource::Points needs [max_items][5] pixel points")),
            },
        };
        let d = self.features;
        let chip = 3 * (IMG_SIZE as usize) * (IMG_SIZE as usize);
        let mut out = ItemEmbeddings {
            features: d,
            embeddings: vec![0f32; m * d],
            valid: vec![0i32; m],
            raw: vec![0f32; if want_raw { m * d } else { 0 }],
            chips: vec![0f32; if want_chips { m * chip } else { 0 }],
        };
        let mut rois = vec![Rect::new(0.5, 0.5, 1.0, 1.0, 0.0, true).to_mi(); m];
        check(unsafe {
            ffi::mi_fe_infer_aligned_items(self.handle, frames.as_ptr(), batch as i32, width, height, stride, source.to_mi(), src, gate,
                                           max_faces as i32, faces.item_frame.as_ptr(), faces.item_face.as_ptr(), m as i32,
                                           out.embeddings.as_mut_ptr(), out.valid.as_mut_ptr(),
                                           if want_raw { out.raw.as_mut_ptr() } else { std::ptr::null_mut() },
                                           if want_chips { out.chips.as_mut_ptr() } else { std::ptr::null_mut() }, rois.as_mut_ptr(),
                                           ffi::MI_MEM_HOST, std::ptr::null_mut())
        })?;
        drop(dets);
        Ok((out, rois.iter().map(Rect::from_mi).collect()))
    }
}

impl Drop for FaceEmbeddings {
    fn drop(&mut self) {
        unsafe { ffi::mi_fe_free(self.handle) }
    }
}

/// The rectangle `crop_image_to_bbox` (face_embeddings.rs:101-109) cuts for `detection.bbox().scale(image_size)`: `(x, y, width, height)`
/// and whether `Mat::roi` takes it (and it is not empty).  Host only.
pub fn face_chip_rect(detection: &Detection, image_size: (i32, i32)) -> Result<((i32, i32, i32, i32), bool), Error> {
    let det = detection.to_mi();
    let mut rect = [0i32; 4];
    let mut valid: i32 = 0;
    check(unsafe { ffi::mi_face_chip_rect(&det, image_size.0, image_size.1, rect.as_mut_ptr(), &mut valid) })?;
    Ok(((rect[0], rect[1], rect[2], rect[3]), valid != 0))
}

/// Where the points of an aligned chip come from (`MI_ALIGN_*`).  Aligned chips are NOT the reference's behaviour: it crops the box.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum AlignSource {
    /// five pixel points: image-left eye, image-right eye, nose tip, image-left and image-right mouth corner
    Points,
    /// the 468 mesh landmarks: eyes = midpoints of 33 / 133 and 362 / 263, nose tip = 1, mouth corners = 61 and 291
    Mesh,
    /// the detection's key points 0..3 (eyes, nose tip, mouth centre) against the four-point template
    Detection,
}

impl AlignSource {
    pub(crate) fn to_mi(self) -> i32 {
        match self {
            AlignSource::Points => ffi::MI_ALIGN_POINTS,
            AlignSource::Mesh => ffi::MI_ALIGN_MESH,
            AlignSource::Detection => ffi::MI_ALIGN_DETECTION,
        }
    }
}

/// The destination points of the aligned chip in chip pixels (`mi_face_align_template`, host only): five, or four for `Detection`.
pub fn face_align_template(source: AlignSource) -> Result<Vec<[f64; 2]>, Error> {
    let mut xy = [[0f64; 2]; 5];
    let mut n: i32 = 0;
    check(unsafe { ffi::mi_face_align_template(source.to_mi(), xy.as_mut_ptr() as *mut f64, &mut n) })?;
    Ok(xy[..n.clamp(0, 5) as usize].to_vec())
}

/// The pixel points of one face by the gather rule (`mi_face_align_points`, host only): `src` is `[468][3]` normalised landmarks for
/// `Mesh`, a detection's 17 floats for `Detection`, `[5][2]` points for `Points`.
pub fn face_align_points(source: AlignSource, src: &[f32], image_size: (i32, i32)) -> Result<Vec<[f32; 2]>, Error> {
    let need = match source {
        AlignSource::Points => 10,
        AlignSource::Mesh => 468 * 3,
        AlignSource::Detection => 17,
    };
    if src.len() != need {
        return Err(Error::msg("the source's operand has another length"));
    }
    let mut pts = [[0f32; 2]; 5];
    let mut n: i32 = 0;
    check(unsafe { ffi::mi_face_align_points(source.to_mi(), src.as_ptr(), image_size.0, image_size.1, pts.as_mut_ptr() as *mut f32, &mut n) })?;
    Ok(pts[..n.clamp(0, 5) as usize].to_vec())
}

/// The least-squares similarity fit of pixel `points` to the template of `source` as the rotated square ROI whose warp to 112 x 112 is the
/// aligned chip, and whether the fit is valid (`mi_face_align_roi`, host only).
pub fn face_align_roi(points: &[[f32; 2]], source: AlignSource) -> Result<(Rect, bool), Error> {
    let mut roi = Rect::new(0.5, 0.5, 1.0, 1.0, 0.0, true).to_mi();
    let mut valid: i32 = 0;
    check(unsafe { ffi::mi_face_align_roi(points.as_ptr() as *const f32, points.len() as i32, source.to_mi(), &mut roi, &mut valid) })?;
    Ok((Rect::from_mi(&roi), valid != 0))
}

/// What `topk_select` and `Gallery::topk` return, `k` slots per query row: slots beyond the eligible rows hold -1 / -inf / -1.
pub struct TopK {
    pub k: usize,
    /// `[n][k]` gallery rows, best first
    pub index: Vec<i32>,
    /// `[n][k]` their scores: bit for bit what `similarity_matrix` gives at `[i][index]`
    pub score: Vec<f32>,
    /// `[n][k]` their labels (`Gallery::topk` only)
    pub label: Vec<i32>,
}

/// The selection rule of `Gallery::topk` applied to a score matrix `[n][m]` (`mi_topk_select`: host only, no GPU).  Row `j` is eligible
/// iff `scores[i][j] > -inf` (NaN and -inf never are); eligible rows by score descending under the plain f32 `>`, ties to the lower `j`.
pub fn topk_select(scores: &[f32], n: usize, m: usize, k: usize) -> Result<TopK, Error> {
    if n == 0 || m == 0 || n.checked_mul(m) != Some(scores.len()) || k == 0 || k > 16 {
        return Err(Error::msg("scores must be [n][m] with n, m >= 1, and k 1..16"));
    }
    let mut out = TopK { k, index: vec![0i32; n * k], score: vec![0f32; n * k], label: Vec::new() };
    check(unsafe { ffi::mi_topk_select(scores.as_ptr(), n as i32, m as i32, k as i32, out.index.as_mut_ptr(), out.score.as_mut_ptr()) })?;
    Ok(out)
}

/// Enrolled embeddings `[m][features]`, copied once into device memory the handle owns, with an `i32` label per row (`None`: the label is
/// the row index).  `topk` answers "who is this": the `k` best rows of every query by cosine score, on the device, without the `[n][m]`
/// score matrix ever reaching memory (`mi_gallery_topk`).
pub struct Gallery {
    handle: *mut ffi::mi_gallery,
    rows: usize,
    features: usize,
}

unsafe impl Send for Gallery {}
unsafe impl Sync for Gallery {}

impl Gallery {
    pub fn new(rows: &[f32], features: usize, labels: Option<&[i32]>) -> Result<Gallery, Error> {
        Self::new_on_device(rows, features, labels, 0)
    }

    pub fn new_on_device(rows: &[f32], features: usize, labels: Option<&[i32]>, device: i32) -> Result<Gallery, Error> {
        if features == 0 || features > 4096 || rows.is_empty() || rows.len() % features != 0 || rows.len() / features > (1 << 24) {
            return Err(Error::msg("rows must be [m][features] with m 1..2^24 and features 1..4096"));
        }
        let m = rows.len() / features;
        if labels.map_or(false, |l| l.len() != m) {
            return Err(Error::msg("one label per row is expected"));
        }
        let mut handle: *mut ffi::mi_gallery = std::ptr::null_mut();
        check(unsafe {
            ffi::mi_gallery_create(device, rows.as_ptr(), m as i32, features as i32, labels.map_or(std::ptr::null(), |l| l.as_ptr()),
                                   ffi::MI_MEM_HOST, &mut handle)
        })?;
        Ok(Gallery { handle, rows: m, features })
    }

    pub fn rows(&self) -> usize {
        self.rows
    }

    pub fn features(&self) -> usize {
        self.features
    }

    /// `"splits"`: the column ranges a row of query tiles is spread over (0 = automatic, the default; otherwise 1..64).  The results do
    /// not depend on it.
    pub fn set_option(&self, key: &str, value: i32) -> Result<(), Error> {
        let key = CString::new(key)?;
        check(unsafe { ffi::mi_gallery_set_option(self.handle, key.as_ptr(), value) })
    }

    pub fn get_option(&self, key: &str) -> Result<i32, Error> {
        let key = CString::new(key)?;
        let mut v: i32 = 0;
        check(unsafe { ffi::mi_gallery_get_option(self.handle, key.as_ptr(), &mut v) })?;
        Ok(v)
    }

    /// `queries` `[n][features]` -> the `k` (1..16) best rows of each.  The embeddings of `FaceEmbeddings::infer_items` are valid queries:
    /// an invalid item (a row of zeros) matches nobody and comes out as all -1.
    pub fn topk(&self, queries: &[f32], k: usize) -> Result<TopK, Error> {
        if queries.is_empty() || queries.len() % self.features != 0 || k == 0 || k > 16 {
            return Err(Error::msg("queries must be [n][features] with n >= 1, and k 1..16"));
        }
        let n = queries.len() / self.features;
        let mut out = TopK { k, index: vec![0i32; n * k], score: vec![0f32; n * k], label: vec![0i32; n * k] };
        check(unsafe {
            ffi::mi_gallery_topk(self.handle, queries.as_ptr(), n as i32, k as i32, out.index.as_mut_ptr(), out.score.as_mut_ptr(),
                                 out.label.as_mut_ptr(), ffi::MI_MEM_HOST, std::ptr::null_mut())
        })?;
        Ok(out)
    }
}

impl Drop for Gallery {
    fn drop(&mut self) {
        unsafe { ffi::mi_gallery_free(self.handle) }
    }
}
