//! The batched detector -> mesh -> iris flow on the device (`mi_pipeline_*`, include/mi_face.h): lib.rs:24-40 of the reference for every
//! frame of a batch — and, with `run_faces`, for every face of a frame — without a host round trip between the stages.
use crate::face_detection::FaceDetectionModel;
use crate::types::Detection;
use crate::{check, ffi};
use anyhow::Error;
use std::ffi::CString;

pub struct Pipeline {
    handle: *mut ffi::mi_pipeline,
}

// libmiface serialises calls on one handle (mi_face.h, conventions)
unsafe impl Send for Pipeline {}
unsafe impl Sync for Pipeline {}

/// What `mi_pipeline_run_faces` returns (host memory).  Item `j < n_items` is face `item_face[j]` of frame `item_frame[j]`; the slots
/// behind hold -1 / -1, `present` 0 and zeros.
pub struct FacesResults {
    /// `[batch][max_faces]`, at most `max_faces` per frame, in the detector's output order
    pub faces: Vec<Vec<Detection>>,
    /// detections the detector found per frame (may exceed `max_faces`)
    pub face_counts: Vec<i32>,
    pub item_frame: Vec<i32>,
    pub item_face: Vec<i32>,
    /// slots used
    pub n_items: usize,
    /// faces (within `max_faces`) that got no slot
    pub dropped: usize,
    /// `[max_items][468][3]`
    pub landmarks: Vec<f32>,
    pub present: Vec<bool>,
    /// `[max_items][2][76][3]`: left eye then right eye, each 71 contour + 5 iris landmarks
    pub eyes: Vec<f32>,
}

/// `mi_face_items_layout` (host only, no GPU): `(item_frame, item_face, n_items, dropped)` of `mi_pipeline_run_faces` for these counts.
pub fn face_items_layout(face_counts: &[i32], max_faces: usize, max_items: usize) -> Result<(Vec<i32>, Vec<i32>, usize, usize), Error> {
    if face_counts.is_empty() || face_counts.len() > i32::MAX as usize || max_faces > i32::MAX as usize || max_items > i32::MAX as usize {
        return Err(Error::msg("face_counts must hold one count per frame"));
    }
    // (the C side writes max_items entries: it refuses max_items beyond 2^20 before it writes, and so must this allocation)
    let slots = max_items.min(1 << 20);
    let (mut item_frame, mut item_face, mut n) = (vec![-1i32; slots], vec![-1i32; slots], [0i32; 2]);
    check(unsafe {
        ffi::mi_face_items_layout(face_counts.as_ptr(), face_counts.len() as i32, max_faces as i32, max_items as i32, item_frame.as_mut_ptr(),
                                  item_face.as_mut_ptr(), n.as_mut_ptr())
    })?;
    Ok((item_frame, item_face, n[0] as usize, n[1] as usize))
}

impl Pipeline {
    /// The detector selected by `model_type` plus face_landmark.tflite and iris_landmark.tflite from `model_dir` (default "./models").
    pub fn new(model_type: FaceDetectionModel, model_dir: Option<String>, device: i32) -> Result<Pipeline, Error> {
        let dir = CString::new(model_dir.unwrap_or_else(|| String::from("./models")))?;
        let mut handle: *mut ffi::mi_pipeline = std::ptr::null_mut();
        check(unsafe { ffi::mi_pipeline_create(model_type as i32, dir.as_ptr(), device, &mut handle) })?;
        Ok(Pipeline { handle })
    }

    /// lib.rs:24-40 for the first `max_faces` (1..16) faces of every frame.  The mesh network runs on exactly `max_items` items and the
    /// iris network on twice as many, whatever the detector finds: choose `max_items` for the faces you expect.
    pub fn run_faces(&self, frames: &[u8], batch: usize, width: i32, height: i32, stride: i32, max_faces: usize, max_items: usize) -> Result<FacesResults, Error> {
        if batch == 0 || batch > (1 << 26) || max_faces == 0 || max_faces > 16 || max_items == 0 || max_items > 32767 || width <= 0 || height <= 0
            || (stride as i64) < 3 * width as i64
        {
            return Err(Error::msg("run_faces: batch 1..2^26, max_faces 1..16, max_items 1..32767, frames of height rows of stride bytes"));
        }
        // the C side reads every frame's rows: a shorter slice must never reach it from safe code
        let (w, h, s) = (width as usize, height as usize, stride as usize);
        let need = s.checked_mul(h).and_then(|f| f.checked_mul(batch - 1)).and_then(|x| x.checked_add(s * (h - 1))).and_then(|x| x.checked_add(3 * w));
        if need.map_or(true, |n| frames.len() < n) {
            return Err(Error::msg("frames must hold batch frames of height rows of stride bytes"));
        }
        let mut faces = vec![ffi::mi_detection { data: [0.0; 16], score: 0.0 }; batch * max_faces];
        let mut face_counts = vec![0i32; batch];
        let (mut item_frame, mut item_face, mut n) = (vec![-1i32; max_items], vec![-1i32; max_items], [0i32; 2]);
        let mut landmarks = vec![0f32; max_items * ffi::MI_NUM_FACE_LANDMARKS * 3];
        let mut present = vec![0i32; max_items];
        let mut eyes = vec![0f32; max_items * 2 * (ffi::MI_NUM_EYE_LANDMARKS + ffi::MI_NUM_IRIS_LANDMARKS) * 3];
        check(unsafe {
            ffi::mi_pipeline_run_faces(self.handle, frames.as_ptr(), batch as i32, width, height, stride, max_faces as i32, max_items as i32,
                                       faces.as_mut_ptr(), face_counts.as_mut_ptr(), item_frame.as_mut_ptr(), item_face.as_mut_ptr(), n.as_mut_ptr(),
                                       landmarks.as_mut_ptr(), present.as_mut_ptr(), eyes.as_mut_ptr(), ffi::MI_MEM_HOST, std::ptr::null_mut())
        })?;
        let faces = (0..batch)
            .map(|b| {
                let k = (face_counts[b].max(0) as usize).min(max_faces);
                faces[b * max_faces..b * max_faces + k].iter().map(Detection::from_mi).collect()
            })
            .collect();
        Ok(FacesResults {
            faces,
            face_counts,
            item_frame,
            item_face,
            n_items: n[0] as usize,
            dropped: n[1] as usize,
            landmarks,
            present: present.iter().map(|&v| v != 0).collect(),
            eyes,
        })
    }
}

impl Drop for Pipeline {
    fn drop(&mut self) {
        unsafe { ffi::mi_pipeline_free(self.handle) }
    }
}
