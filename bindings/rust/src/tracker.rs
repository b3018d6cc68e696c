//! Landmark-to-ROI face tracking for video streams (`mi_tracker_*`, include/mi_face.h).  NOT the reference's behaviour — the reference has
//! no video loop.  This is MediaPipe's: the ROI of a stream's next frame comes from the landmarks of its last one, and the detector runs
//! only for streams that have no face yet or have lost it, composed from the reference's own `bbox_from_landmarks` and `bbox_to_roi`.
use crate::face_detection::FaceDetectionModel;
use crate::types::{Detection, Rect};
use crate::{check, ffi};
use anyhow::Error;
use std::ffi::CString;

pub struct Tracker {
    handle: *mut ffi::mi_tracker,
    streams: usize,
}

// libmiface serialises calls on one handle (mi_face.h, conventions); a handle's steps are ordered
unsafe impl Send for Tracker {}
unsafe impl Sync for Tracker {}

/// What `mi_tracker_step` returns (host memory), one entry per stream.
pub struct TrackStep {
    /// the detection a stream was acquired from (`source == 1`)
    pub faces: Vec<Option<Detection>>,
    /// the detector's count for a stream that held a slot, else 0
    pub face_counts: Vec<i32>,
    /// 2: the state's ROI, 1: the detector's, 0: none
    pub source: Vec<i32>,
    /// the ROI the mesh ran on (`None` for source 0)
    pub rois: Vec<Option<Rect>>,
    /// `[streams][468][3]`
    pub landmarks: Vec<f32>,
    pub present: Vec<bool>,
    /// `[streams][2][76][3]`: left eye then right eye, each 71 contour + 5 iris landmarks
    pub eyes: Vec<f32>,
    /// `[max_detect]`: the stream of every detector slot, -1 when unused
    pub det_stream: Vec<i32>,
    /// slots used
    pub n_detect: usize,
    /// lost streams left without a slot
    pub waiting: usize,
}

fn zero_rect() -> ffi::mi_rect {
    ffi::mi_rect { x_center: 0.0, y_center: 0.0, width: 0.0, height: 0.0, rotation: 0.0, normalized: 0 }
}

/// `mi_track_roi_from_landmarks` (host only, no GPU): the ROI a tracker derives for the next frame from `[468][3]` landmarks normalised to
/// a frame of `image_size = (width, height)`; `None` for an invalid set.
pub fn track_roi_from_landmarks(landmarks: &[f32], image_size: (i32, i32)) -> Result<Option<Rect>, Error> {
    if landmarks.len() != ffi::MI_NUM_FACE_LANDMARKS * 3 {
        return Err(Error::msg("landmarks must be [468][3]"));
    }
    let (mut roi, mut valid) = (zero_rect(), 0i32);
    check(unsafe { ffi::mi_track_roi_from_landmarks(landmarks.as_ptr(), image_size.0, image_size.1, &mut roi, &mut valid) })?;
    Ok(if valid != 0 { Some(Rect::from_mi(&roi)) } else { None })
}

/// `mi_track_detect_layout` (host only, no GPU): `(det_stream, slots used, lost streams left without a slot)` of a step.
pub fn track_detect_layout(tracked: &[i32], max_detect: usize, start: usize) -> Result<(Vec<i32>, usize, usize), Error> {
    if tracked.is_empty() || tracked.len() > (1 << 20) || max_detect == 0 || max_detect > tracked.len() || start >= tracked.len() {
        return Err(Error::msg("track_detect_layout: streams 1..2^20, max_detect 1..streams, start 0..streams-1"));
    }
    let (mut det_stream, mut n) = (vec![-1i32; max_detect], [0i32; 2]);
    check(unsafe {
        ffi::mi_track_detect_layout(tracked.as_ptr(), tracked.len() as i32, max_detect as i32, start as i32, det_stream.as_mut_ptr(), n.as_mut_ptr())
    })?;
    Ok((det_stream, n[0] as usize, n[1] as usize))
}

impl Tracker {
    /// `streams` (1..32767) video streams on the detector selected by `model_type` plus face_landmark.tflite and iris_landmark.tflite from
    /// `model_dir` (default "./models").  Every stream starts lost.
    pub fn new(model_type: FaceDetectionModel, streams: usize, model_dir: Option<String>, device: i32) -> Result<Tracker, Error> {
        if streams == 0 || streams > 32767 {
            return Err(Error::msg("streams must be 1..32767"));
        }
        let dir = CString::new(model_dir.unwrap_or_else(|| String::from("./models")))?;
        let mut handle: *mut ffi::mi_tracker = std::ptr::null_mut();
        check(unsafe { ffi::mi_tracker_create(model_type as i32, dir.as_ptr(), device, streams as i32, &mut handle) })?;
        Ok(Tracker { handle, streams })
    }

    pub fn streams(&self) -> usize {
        self.streams
    }

    pub fn set_option(&self, key: &str, value: i32) -> Result<(), Error> {
        let key = CString::new(key)?;
        check(unsafe { ffi::mi_tracker_set_option(self.handle, key.as_ptr(), value) })
    }

    /// One step: `frames` holds one RGB frame per stream, frame `s` the next picture of stream `s`.  The detector runs on exactly
    /// `max_detect` (1..streams) items, the mesh on `streams` and the iris network on twice as many.
    pub fn step(&self, frames: &[u8], width: i32, height: i32, stride: i32, max_detect: usize) -> Result<TrackStep, Error> {
        let n = self.streams;
        if max_detect == 0 || max_detect > n || width <= 0 || height <= 0 || (stride as i64) < 3 * width as i64 {
            return Err(Error::msg("step: max_detect 1..streams, frames of height rows of stride bytes"));
        }
        // the C side reads every frame's rows: a shorter slice must never reach it from safe code
        let (w, h, s) = (width as usize, height as usize, stride as usize);
        let need = s.checked_mul(h).and_then(|f| f.checked_mul(n - 1)).and_then(|x| x.checked_add(s * (h - 1))).and_then(|x| x.checked_add(3 * w));
        if need.map_or(true, |b| frames.len() < b) {
            return Err(Error::msg("frames must hold one frame per stream of height rows of stride bytes"));
        }
        let mut faces = vec![ffi::mi_detection { data: [0.0; 16], score: 0.0 }; n];
        let (mut face_counts, mut source, mut present) = (vec![0i32; n], vec![0i32; n], vec![0i32; n]);
        let mut rois: Vec<ffi::mi_rect> = (0..n).map(|_| zero_rect()).collect();
        let mut landmarks = vec![0f32; n * ffi::MI_NUM_FACE_LANDMARKS * 3];
        let mut eyes = vec![0f32; n * 2 * (ffi::MI_NUM_EYE_LANDMARKS + ffi::MI_NUM_IRIS_LANDMARKS) * 3];
        let (mut det_stream, mut n_detect) = (vec![-1i32; max_detect], [0i32; 2]);
        check(unsafe {
            ffi::mi_tracker_step(self.handle, frames.as_ptr(), width, height, stride, max_detect as i32, faces.as_mut_ptr(), face_counts.as_mut_ptr(),
                                 source.as_mut_ptr(), rois.as_mut_ptr(), landmarks.as_mut_ptr(), present.as_mut_ptr(), eyes.as_mut_ptr(),
                                 det_stream.as_mut_ptr(), n_detect.as_mut_ptr(), ffi::MI_MEM_HOST, std::ptr::null_mut())
        })?;
        Ok(TrackStep {
            faces: (0..n).map(|i| if source[i] == 1 { Some(Detection::from_mi(&faces[i])) } else { None }).collect(),
            face_counts,
            rois: (0..n).map(|i| if source[i] != 0 { Some(Rect::from_mi(&rois[i])) } else { None }).collect(),
            source,
            landmarks,
            present: present.iter().map(|&v| v != 0).collect(),
            eyes,
            det_stream,
            n_detect: n_detect[0] as usize,
            waiting: n_detect[1] as usize,
        })
    }

    /// Drops the state of one stream, or of all (`None`: the detect plan then starts at stream 0 again).
    pub fn reset(&self, stream_index: Option<usize>) -> Result<(), Error> {
        let i = match stream_index {
            Some(i) if i < self.streams => i as i32,
            Some(_) => return Err(Error::msg("reset: no such stream")),
            None => -1,
        };
        check(unsafe { ffi::mi_tracker_reset(self.handle, i) })
    }

    /// The state: per stream its ROI while it is tracked, `None` while it is lost.
    pub fn state(&self) -> Result<Vec<Option<Rect>>, Error> {
        let mut rois: Vec<ffi::mi_rect> = (0..self.streams).map(|_| zero_rect()).collect();
        let mut tracked = vec![0i32; self.streams];
        check(unsafe { ffi::mi_tracker_get_state(self.handle, rois.as_mut_ptr(), tracked.as_mut_ptr()) })?;
        Ok((0..self.streams).map(|i| if tracked[i] != 0 { Some(Rect::from_mi(&rois[i])) } else { None }).collect())
    }

    /// Writes the state of streams `first .. first + state.len() - 1`.
    pub fn set_state(&self, first: usize, state: &[Option<Rect>]) -> Result<(), Error> {
        if state.is_empty() || first >= self.streams || state.len() > self.streams - first {
            return Err(Error::msg("set_state: first and the state's length must name streams of the handle"));
        }
        let rois: Vec<ffi::mi_rect> = state.iter().map(|r| r.map_or_else(zero_rect, |r| r.to_mi())).collect();
        let tracked: Vec<i32> = state.iter().map(|r| r.is_some() as i32).collect();
        check(unsafe { ffi::mi_tracker_set_state(self.handle, first as i32, state.len() as i32, rois.as_ptr(), tracked.as_ptr()) })
    }
}

impl Drop for Tracker {
    fn drop(&mut self) {
        unsafe { ffi::mi_tracker_free(self.handle) }
    }
}
