// What another handle of libsdrx.so needs to run behind a channel back-end it owns (sdrx_am.hip): the device-side view of a
// channel's last outputs without a host round trip, and the stream the back-end launches on.
#pragma once
#include "sdrx_common.hpp"

namespace sdrx {

struct BackendView {
    const void* out;        // float2 (no discriminator) or float samples of the last feed; may move when a feed grows the buffers
    const int* n_out;       // their count, written on the device by the feed's last kernel
};
int backend_view(sdrx_backend_t* b, int32_t ch, BackendView* v);
// sdrx_backend_create with the Interpolator's cutoff of channel c as the double cutoff[c] in place of cfg[c].interp_cutoff:
// for a caller whose reference passes Interpolator::create a double that no float holds (LoRaDemod: m_Bandwidth / 1.9).
int backend_create_cutoff(sdrx_backend_t** out, int device, int32_t n_ch, const sdrx_backend_cfg* cfg, const double* cutoff);
// hip_stream == nullptr: back to the back-end's own stream.  Waits for the work queued so far.
int backend_set_stream(sdrx_backend_t* b, hipStream_t hip_stream);
// A back-end that has not been fed yet: channel ch resamples with this distance step (UDPSrc divides by a float rate) and its
// m_sampleDistanceRemain starts at `distance` instead of 0 (UDPSrc starts at one step).  step >= 1, distance >= 0.
int backend_start_at(sdrx_backend_t* b, int32_t ch, float step, float distance);
// A back-end that has not been fed yet: channel ch runs without the Interpolator (bypass: every NCO-mixed sample is a filter
// input, as ChannelAnalyzer does with m_useInterpolator off) and / or with NCOF, the oscillator with a float phase and a float
// increment (ncof.h), in place of NCO.
int backend_set_front(sdrx_backend_t* b, int32_t ch, int bypass, int ncof);
// A back-end that has not been fed yet: channel ch runs without an oscillator, the int16 sample itself is what the NCO mix
// would have produced.  ATVDemod::feed skips the mix when the offset is 0, and NCO::nextIQ at phase 0 is (1, -cos(pi / 2)) with
// the cosine rounded to 6.1e-17, so the product is not the sample where its real or imaginary part is 0.
int backend_set_nomix(sdrx_backend_t* b, int32_t ch);

} // namespace sdrx
