// The block schedule of UDPSrc::feed's SSB formats (FormatLSB, FormatUSB, FormatLSBMono, FormatUSBMono; udpsrc.cpp:179-242)
// in closed form.  fftfilt::runSSB (fftfilt.cpp:285-325) with flen 512 collects 256 resampled samples, inptr counting them
// across feeds, and hands out a block of 256 in the call that brings the 256th: the block is written to the UDPSink in the
// loop iteration of that sample, after its calculateSquelch.  FormatLSB's `if` is not chained to the else-if ladder behind it,
// so with format 4 that ladder ends in its raw I/Q branch: every resampled sample, after any block it completed, also
// writes one raw element to the same sink.  With `pending` = inptr before a feed of n resampled samples, indices k counted
// within the feed and blocks b counted within the feed, everything below follows.  Compiles for the host too
// (tests/udpsrc_ssb_scan_check.cpp), no HIP header needed.
#pragma once
#include "udpsrc_scan.hpp"

namespace sdrx {

constexpr int UDP_SSB_FLEN = 512;                           // UDPSrc::udpBlockSize
constexpr int UDP_SSB_H = UDP_SSB_FLEN / 2;                 // flen2: samples per block

AM_HD bool udp_fmt_ssb(int fmt) { return fmt >= UDP_LSB && fmt <= UDP_USB_MONO; }
AM_HD bool udp_fmt_ssb_usb(int fmt) { return fmt == UDP_USB || fmt == UDP_USB_MONO; }
AM_HD bool udp_fmt_ssb_mono(int fmt) { return fmt == UDP_LSB_MONO || fmt == UDP_USB_MONO; }

AM_HD int udp_ssb_blocks(int pending, int n) { return (int)(((long)pending + n) / UDP_SSB_H); }       // blocks the feed completes
AM_HD int udp_ssb_left(int pending, int n) { return (int)(((long)pending + n) % UDP_SSB_H); }         // inptr after the feed
AM_HD int udp_ssb_completing(int pending, int b) { return (b + 1) * UDP_SSB_H - pending - 1; }        // the sample that fills block b
AM_HD int udp_ssb_blocks_through(int pending, int k) { return (int)(((long)pending + k + 1) / UDP_SSB_H); }   // blocks completed by samples 0 .. k
// input j of block b, as an index into the feed; negative: carried sample `pending + index`
AM_HD int udp_ssb_source(int pending, int b, int j) { return b * UDP_SSB_H + j - pending; }
// carried sample i of the next feed (i < udp_ssb_left): the same rule one block further
AM_HD int udp_ssb_carried_source(int pending, int n, int i) { return udp_ssb_source(pending, udp_ssb_blocks(pending, n), i); }

// payload positions within the feed, in elements.  Format 4: raw sample k sits behind the k raw elements before it and every
// block completed through k; block b sits right in front of its completing sample's raw element.  Formats 5 .. 7: blocks only.
AM_HD long udp_ssb_raw_pos(int pending, int k) { return (long)k + (long)UDP_SSB_H * udp_ssb_blocks_through(pending, k); }
AM_HD long udp_ssb_block_pos(int fmt, int pending, int b)
{
    return fmt == UDP_LSB ? (long)udp_ssb_completing(pending, b) + (long)UDP_SSB_H * b : (long)UDP_SSB_H * b;
}
AM_HD long udp_ssb_payload_count(int fmt, int pending, int n)
{
    return (fmt == UDP_LSB ? (long)n : 0) + (long)UDP_SSB_H * udp_ssb_blocks(pending, n);
}
// most payload elements a feed of n resampled samples can have, whatever was pending
AM_HD long udp_ssb_payload_bound(long n) { return 2 * n + UDP_SSB_H; }

} // namespace sdrx
