// ofdm_hip_tuning.h -- the laboratory keys of ofdm_set_tuning / ofdm_get_tuning (PRIVATE: tools/, tests/ and ofdm_abi.hip; not part of
// the drop-in contract of include/ofdm_hip.h, free to change between rounds).  One line per key: OFDM_TUNE_KEY(name, Tuning field,
// profile-build-only).  ofdm_abi.hip expands the list into its key table; value checks for keys that size LDS tiles or pick template
// instantiations are in ofdm_set_tuning.
//
//   A/B between kernel families (1 = take the older / generic kernel instead)
//     no_sc80             N = 64, W = 3 L Schmidl-Cox: the f32 filter pair k_sc_cf<128,first> + k_sc_cf<256,list> instead of k_sc80
//     no_sc_stream        L = 160 .. 5120: k_scb_chunks + k_scb_fine / k_sc_tile instead of the streaming detector k_sc_stream
//     no_sc_big           long periods through k_sc_tile instead of k_scb_chunks + k_scb_fine
//     no_fast64, no_demod4096, no_mid_kernels, no_rxframe1024, no_txframe64     the generic k_sym instead of that family
//     no_rx1024_finish    k_rxframe1024 writes raw bytes and k_rx_finish runs as its own launch
//     no_rxframe64_split  k_rxframe64 as one kernel with both frame bodies instead of the common-body / cut-body pair
//   shapes and depths
//     sc80_depth          k_sc80: steps between the last read of a ring piece and its refill (2: 7 KiB in flight per wavefront, 1: 9-10)
//     sc_wg_per_cu, sc_first_lags, sc128_one_wave                     k_sc_cf (the filter pair): workgroups per CU, lags of the first
//                         launch (0 = one launch), one wavefront per frame in the 128-chunk kernel
//     demod64_wg_per_cu, demod64_burst (16 / 8 / 4 / 1), demod64_narrow_stores,  k_demod64
//     demod64_store_policy (0, 1 nt, 2 sc1, 3 sc0 sc1)
//     tx_waves, txframe_keep_steps, txframe_rewrite,                  k_txframe64 / k_txframe_mid / k_txframe4096
//     no_txframe_optimistic
//     scb_two_segments, scb_big_tiles                                 k_scb_chunks / k_scb_fine
//   soft decode (OFDM_ECC_HAMMING74_SOFT, OFDM_ECC_CONV_K7)
//     soft_chunk_frames   frames per k_sym<llr> + k_rx_finish_soft / k_viterbi_k7 step of the decode chain (0 = as many as fit the 256 MB LLR workspace;
//                         the tests force a few frames to walk many steps)
//   channel-estimate denoising (EXT-5)
//     chest_solve_only    ofdm_chest_smooth_batch launches k_chest_solve alone on the rows it is given, into its workspace, and delivers
//                         nothing: the kernel's time on its own (tools/bench_chest.py)
//   frame check (OFDM_ECC_FCS + mode)
//     fcs_bitserial       k_fcs_wrap / k_fcs_check reduce every lane's chunk bit by bit in registers instead of through the slice-by-4
//                         tables in LDS (tools/bench_fcs.py times both)
//   sc16 receive input (EXT-9)
//     no_demod64_sc16     ofdm_rx_demod_sc16_batch at N = 64 inside the fused kernel's envelope: k_sc16_widen into the workspace + the fc32
//                         path instead of k_demod64_sc16 (tools/bench_sc16.py times both)
//     sc16_chunk_frames   frames per k_sc16_widen + fc32 chain step of ofdm_rx_demod_sc16_batch's widen path and of
//                         ofdm_rx_decode_sc16_batch (0 = about 48 MB of widened samples; the tests put chunk boundaries inside five frames);
//                         also (EXT-10) frames per fc32 encode + k_sc16_narrow step of ofdm_tx_encode_sc16_batch's two-pass path
//   sc16 transmit output (EXT-10)
//     no_txframe64_sc16   ofdm_tx_encode_sc16_batch at N = 64 inside the fused kernel's envelope: the fc32 encode chain into the workspace +
//                         k_sc16_narrow instead of k_txframe64_sc16 (tools/bench_sc16_tx.py times both)
//   every detection of a long capture (EXT-12)
//     scan_mark_only      ofdm_sc_scan_long launches k_sc_mark alone over its lag range and reports no detection: the kernel's time on
//                         its own (tools/bench_scan.py)
//   every packet of a long capture in one batched decode (EXT-13)
//     packets_chunk_rows  packets per k_gather_rows + chain step of ofdm_rx_decode_packets (0 = as many as keep the gathered rows within
//                         256 MiB; the tests force chunks of 2 rows)
//     packets_gather_only ofdm_rx_decode_packets launches k_pkt_rows + k_gather_rows alone and delivers nothing: the gather's time on its
//                         own (tools/bench_packets.py)
//   a streaming receiver (EXT-14)
//     stream_scan_cap     detections per scan + decode round of ofdm_stream_push (0 or above 256 = 256; the tests force 2, so that a push
//                         walks several rounds and resumes each behind the last detection of the one before)
//   Schmidl-Cox threshold in full precision (handled by name in ofdm_abi.hip, 64 bits: not in the table below)
//     sync_threshold_bits the bit pattern of a double in (0, 1] that replaces ofdm_params.sync_threshold (a float: 6e-8 apart) in every
//                         search of the context; 0 = the float again.  The margin tests set the threshold within 1e-12 of a lag's own metric
//   what the workspaces hold (handled by name in ofdm_abi.hip: not in the table below; tests/test_gpu_ws_poison.py, DESIGN.md "the
//   workspace ledger")
//     ws_poison           0 = off: nothing is ever filled, the code of every path is what it is without the key.  0x100 + b (b = 0 .. 255) = on
//                         with fill byte b; every other value: OFDM_ERR_INVALID.  Setting it on synchronises the context's stream (and the
//                         host pipe's, if there is one) and fills, once, every workspace that holds memory and every device and pinned
//                         buffer of the host pipe over its whole capacity with b.  While it is on every GROWTH (ws_get, and the pipe's dev_grow
//                         / pin_grow) fills the new allocation over its capacity before handing it out; an ordinary ws_get fills nothing (an
//                         entry point may take a role more than once).  A fill is a memset, no launch: the dispatch strings do not change
//     stat_ws_roles       get: kWsRoles, the number of workspace roles (WsRole, ofdm_ctx.hpp)
//     stat_ws_live        get: bit r is set when role r holds memory
//     stat_ws_ptr:<r>, stat_ws_cap:<r>   get: the device address and the capacity in bytes of role r (0 and 0 when it holds nothing); with
//                         ofdm_memcpy_d2h the tests read a workspace back whole
//     stat_pipe_bufs, stat_pipe_ptr:<i>, stat_pipe_cap:<i>, stat_pipe_pinned:<i>   get: the same for the host pipe's buffers (the device
//                         slots, the long-capture copies and scalars, then the pinned slots): how many there are, and of buffer i the
//                         address, the capacity and whether it is pinned host memory (all 0 before the first host-buffer call)
//   profile build only (libofdm_hip_profile.so): ablation exits and s_memtime section timers
//     debug_demod64, debug_sc, debug_tx
#ifndef OFDM_TUNE_KEY
#error "define OFDM_TUNE_KEY(name, field, profile_only) before including ofdm_hip_tuning.h"
#endif
OFDM_TUNE_KEY("no_sc80", no_sc80, false)
OFDM_TUNE_KEY("sc80_depth", sc80_depth, false)
OFDM_TUNE_KEY("no_sc_stream", no_sc_stream, false)
OFDM_TUNE_KEY("no_sc_big", no_sc_big, false)
OFDM_TUNE_KEY("no_fast64", no_fast64, false)
OFDM_TUNE_KEY("no_demod4096", no_demod4096, false)
OFDM_TUNE_KEY("no_mid_kernels", no_mid_kernels, false)
OFDM_TUNE_KEY("no_rxframe1024", no_rxframe1024, false)
OFDM_TUNE_KEY("no_txframe64", no_txframe64, false)
OFDM_TUNE_KEY("no_rx1024_finish", no_rx1024_finish, false)
OFDM_TUNE_KEY("no_rxframe64_split", no_rxframe64_split, false)
OFDM_TUNE_KEY("tx_waves", tx_waves, false)
OFDM_TUNE_KEY("txframe_keep_steps", txframe_keep_steps, false)
OFDM_TUNE_KEY("txframe_rewrite", txframe_rewrite, false)
OFDM_TUNE_KEY("no_txframe_optimistic", no_txframe_optimistic, false)
OFDM_TUNE_KEY("sc_wg_per_cu", sc_wg_per_cu, false)
OFDM_TUNE_KEY("sc_first_lags", sc_first_lags, false)
OFDM_TUNE_KEY("sc128_one_wave", sc128_one_wave, false)
OFDM_TUNE_KEY("demod64_wg_per_cu", demod64_wg_per_cu, false)
OFDM_TUNE_KEY("demod64_burst", demod64_burst, false)
OFDM_TUNE_KEY("demod64_narrow_stores", demod64_narrow_stores, false)
OFDM_TUNE_KEY("demod64_store_policy", demod64_store_policy, false)
OFDM_TUNE_KEY("scb_two_segments", scb_two_segments, false)
OFDM_TUNE_KEY("scb_big_tiles", scb_big_tiles, false)
OFDM_TUNE_KEY("soft_chunk_frames", soft_chunk_frames, false)
OFDM_TUNE_KEY("chest_solve_only", chest_solve_only, false)
OFDM_TUNE_KEY("fcs_bitserial", fcs_bitserial, false)
OFDM_TUNE_KEY("no_demod64_sc16", no_demod64_sc16, false)
OFDM_TUNE_KEY("sc16_chunk_frames", sc16_chunk_frames, false)
OFDM_TUNE_KEY("no_txframe64_sc16", no_txframe64_sc16, false)
OFDM_TUNE_KEY("scan_mark_only", scan_mark_only, false)
OFDM_TUNE_KEY("packets_chunk_rows", packets_chunk_rows, false)
OFDM_TUNE_KEY("packets_gather_only", packets_gather_only, false)
OFDM_TUNE_KEY("stream_scan_cap", stream_scan_cap, false)
OFDM_TUNE_KEY("debug_demod64", debug_demod64, true)
OFDM_TUNE_KEY("debug_sc", debug_sc, true)
OFDM_TUNE_KEY("debug_tx", debug_tx, true)
