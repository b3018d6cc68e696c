//! utils.rs:8-50 of the reference: `convert_image_to_mat(im_bytes)` for JPEG input — Huffman decoding on the host, IDCT /
//! chroma upsampling / colour conversion on the GPU, bit-identical to libjpeg-turbo (what `cv::imdecode` runs) — and `l2_norm` /
//! `similarity_score`, bit-identical to the reference's order of operations.
use crate::{check, ffi};
use anyhow::Error;

/// Owning 8UC3 RGB picture (what the reference holds as a `Mat`); `infer(&picture, ..)` borrows it through
/// `TryFrom<&RgbImage> for Image`.  Private fields: the buffer always matches the geometry.
pub struct RgbImage {
    data: Vec<u8>,
    width: i32,
    height: i32,
}

impl RgbImage {
    pub fn new(data: Vec<u8>, width: i32, height: i32) -> Result<RgbImage, Error> {
        if width <= 0 || height <= 0 || data.len() != 3 * width as usize * height as usize {
            return Err(Error::msg("RGB buffer does not match width x height x 3"));
        }
        Ok(RgbImage { data, width, height })
    }
    pub fn data(&self) -> &[u8] {
        &self.data
    }
    pub fn width(&self) -> i32 {
        self.width
    }
    pub fn height(&self) -> i32 {
        self.height
    }
    pub fn image(&self) -> crate::types::Image<'_> {
        crate::types::Image { data: &self.data, width: self.width, height: self.height, stride: 3 * self.width }
    }
}

/// Baseline / extended-sequential / progressive Huffman JPEG, 8 bit, grey or YCbCr (h1v1, h2v1, h2v2).  Anything else (
/// arithmetic coding, other containers) is an error: keep `imdecode` for those ("Pictures libmiface does not
/// decode": fall back to the reference's own `convert_image_to_mat` and pass the `Mat` to `infer` under `--features opencv`).
pub fn convert_image_to_mat(im_bytes: &[u8]) -> Result<RgbImage, Error> {
    let (mut w, mut h) = (0i32, 0i32);
    check(unsafe { ffi::mi_jpeg_info(im_bytes.as_ptr(), im_bytes.len(), &mut w, &mut h) })?;
    let mut data = vec![0u8; 3 * w as usize * h as usize];
    check(unsafe {
        ffi::mi_jpeg_decode_rgb(0, im_bytes.as_ptr(), im_bytes.len(), data.as_mut_ptr(), data.len(), &mut w, &mut h, ffi::MI_MEM_HOST,
                                std::ptr::null_mut())
    })?;
    Ok(RgbImage { data, width: w, height: h })
}

/// `l2_norm(arr)` — utils.rs:30-33: `arr / sqrt(sum of squares)`, the sum in f32 and in index order.  The reference takes an
/// `Array2<f32>` and normalises it as a whole; the `[1, D]` array is its row here.
pub fn l2_norm(arr: &[f32]) -> Result<Vec<f32>, Error> {
    if arr.is_empty() || arr.len() > i32::MAX as usize {
        return Err(Error::msg("l2_norm: 1 .. 2^31 - 1 values are expected"));
    }
    let mut out = vec![0f32; arr.len()];
    check(unsafe { ffi::mi_l2_norm(arr.as_ptr(), arr.len() as i32, out.as_mut_ptr()) })?;
    Ok(out)
}

/// `similarity_score(a, b)` — utils.rs:44-50: the cosine of two vectors, all three sums f32 and sequential.  The reference zips the two
/// vectors (a length mismatch silently shortens the dot product only); here it is a panic, like any other contract violation of a
/// function that returns a bare `f32`.
pub fn similarity_score(a: &Vec<f32>, b: &Vec<f32>) -> f32 {
    assert!(a.len() == b.len() && !a.is_empty() && a.len() <= i32::MAX as usize, "similarity_score: two vectors of one length");
    let mut out = 0f32;
    let rc = unsafe { ffi::mi_similarity_score(a.as_ptr(), b.as_ptr(), a.len() as i32, &mut out) };
    assert!(rc == ffi::MI_OK, "mi_similarity_score failed");
    out
}

/// `similarity_score` of every row of `a` (`[n][features]`) against every row of the gallery `b` (`[m][features]`) on the GPU's f32
/// matrix cores (`mi_similarity_matrix`): `[n][m]`, host memory.
pub fn similarity_matrix(a: &[f32], b: &[f32], features: usize, device: i32) -> Result<Vec<f32>, Error> {
    if features == 0 || features > 4096 || a.is_empty() || b.is_empty() || a.len() % features != 0 || b.len() % features != 0 {
        return Err(Error::msg("similarity_matrix: rows of 1..4096 features are expected"));
    }
    let (n, m) = (a.len() / features, b.len() / features);
    if n > i32::MAX as usize || m > i32::MAX as usize {
        return Err(Error::msg("similarity_matrix: too many rows"));
    }
    let mut out = vec![0f32; n * m];
    check(unsafe {
        ffi::mi_similarity_matrix(device, a.as_ptr(), n as i32, b.as_ptr(), m as i32, features as i32, out.as_mut_ptr(), ffi::MI_MEM_HOST,
                                  std::ptr::null_mut())
    })?;
    Ok(out)
}
