// Sample coordinates of tf.image.crop_and_resize (TF-1.3 crop_and_resize_op.cc): the one place they are written.
// crop_kernel (crop.hip) samples at them and the correlation's tile-list builder (correlation.hip) bounds them, so
// the two cannot disagree about which pixels a crop reads.
#pragma once

namespace dodt {

// Coordinate, in pixels of an axis of `size` pixels, of sample i of `crop` samples between the normalised box edges
// lo and hi.  (Built with -ffp-contract=off: the products and sums stay separate roundings.)
__device__ __forceinline__ float crop_coord(float lo, float hi, int size, int crop, int i) {
    const float m1 = (float)(size - 1);
    const float step = (crop > 1) ? (hi - lo) * m1 / (float)(crop - 1) : 0.0f;
    return (crop > 1) ? lo * m1 + (float)i * step : 0.5f * (lo + hi) * m1;
}

}  // namespace dodt
