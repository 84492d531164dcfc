/* libwfae.so — forecast verification per lead time (csrc/verify.hip).
 *
 * Part of the C ABI of include/wfae.h, which includes this file inside its extern "C" block: a C or C++ caller includes
 * wfae.h and never this file alone (it uses wfae.h's wfae_stream_t and status codes).  The conventions are wfae.h's:
 * device pointers unless marked HOST, the stream last, 0 on success, a negative wfae_status otherwise, the message in
 * wfae_last_error_string().  Added within ABI version 103; nothing else changed. */
#ifndef WFAE_VERIFY_H
#define WFAE_VERIFY_H

/* ---- forecast verification per lead time (csrc/verify.hip): F <= 4 fields scored against one target in one pass.
 * A field is (device pointer, elements between samples, elements between leads); `fields`, `field_bstride`,
 * `field_lstride` and `thresholds` (n_thr <= 8) are HOST arrays.  A lead stride of 0 is the same frame at every lead
 * (persistence).  The S = C*H*W pixels of one frame are contiguous; nothing else about the layout is assumed and nothing
 * is copied.  Bases and strides need no alignment: 16-byte loads are used when S % 4 == 0 and every base and stride is
 * 16-byte aligned, dword loads otherwise.  clamp01 != 0 clamps field and target values to [0, 1] in fp32 first; an event
 * is `value >= threshold` in fp32; e = (double)field - (double)target.  Inputs must be finite (not checked).
 * counts (device, P x F x (3 n_thr + 1) int64): [tp, fn, fp] per threshold, then the cell count B * S of the lead.
 * sums (device, P x F x 2 double): sum e^2, sum |e|.  accumulate != 0 adds to both tables, else they are overwritten.
 * No atomics: blocks write partial rows, the finalize kernel adds them in ascending block order, so the same inputs give
 * the same bits.  ws: >= P * min(256, ceil(B * S / 1024)) * F * (3 n_thr + 2) * 8 bytes.
 * rc: -2 for a null pointer, -1 for F outside [1, 4], n_thr outside [0, 8], B, P or S < 1, B * P * S > 2^40, a negative
 * stride, or a workspace below the formula. */
int wfae_verify_leads(const float* const* fields, const int64_t* field_bstride, const int64_t* field_lstride,
                      const float* target, int64_t target_bstride, int64_t target_lstride, int F, int B, int P, int64_t S,
                      const float* thresholds, int n_thr, int clamp01, int accumulate, int64_t* counts, double* sums,
                      void* ws, size_t ws_bytes, wfae_stream_t stream);

#endif /* WFAE_VERIFY_H */
