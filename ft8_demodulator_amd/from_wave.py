"""The reference's decode-a-WAV entry point (src/tests/demodulator/from_wave.py:24-234), drop-in.

read_wave_file keeps the reference semantics (stdlib `wave`, widths 1/2/4 -> uint8/int16/int32,
channel 0 of stereo, float32 / iinfo.max).  decode_ft8_from_wave uploads 16-bit PCM as int16 and
lets the STFT kernel apply the float32 x/32767 scaling on the device (bit-identical to
read_wave_file, half the host->device bytes); other widths are converted on the host as the
reference does.  `python -m ft8_demodulator_amd.from_wave file.wav [flags]` is the CLI.
"""
from __future__ import annotations

import argparse
import os
import sys
import wave

import numpy as np


def _read_raw(wave_path: str, verbose: bool = False):
    with wave.open(wave_path, "rb") as wf:
        n_channels = wf.getnchannels()
        sample_width = wf.getsampwidth()
        sample_rate = wf.getframerate()
        n_frames = wf.getnframes()
        if verbose:
            print(f"n_channels: {n_channels}")
            print(f"sample_width: {sample_width}")
            print(f"sample_rate: {sample_rate}")
            print(f"n_frames: {n_frames}")
        raw = wf.readframes(n_frames)
    if sample_width == 1:
        dtype = np.uint8
    elif sample_width == 2:
        dtype = np.int16
    elif sample_width == 4:
        dtype = np.int32
    else:
        raise ValueError(f"Unsupported sample width: {sample_width}")
    data = np.frombuffer(raw, dtype=dtype)
    if n_channels == 2:
        data = data[::2]
    return data, dtype, sample_rate


def read_wave_file(wave_path: str, verbose: bool = False) -> tuple:
    """from_wave.py:24-69 -> (float32 samples in [-1, 1], sample_rate)."""
    data, dtype, sample_rate = _read_raw(wave_path, verbose)
    x = data.astype(np.float32)
    x /= np.iinfo(dtype).max
    return x, sample_rate


def _decode_file(wave_path: str, *, snr: bool = False, ap=None, ap_max_hard_errors: int = None, coherent=None,
                 coherent_drift=None, coherent_nsym: int = 1, selection: str = "reference", subtract=None,
                 coherent_ap: bool = False, osd=None, osd_max_hard_errors: int = None, device=None,
                 verbose: bool = False, **decode_kw) -> tuple:
    """One file, any PCM width, as one slot through _pipeline.decode_one -> (results, snr_db, patterns)
    and, with coherent, a fourth entry.  snr_db (with snr, else None): one SNR in 2500 Hz per result.
    patterns (with ap, else None): per result the a-priori pattern that rescued it, None for a plain
    decode.  fits (with coherent): per result (dt_s, df_hz) of the coherent fit that rescued it (one
    ft8_coherent_llr call for those records), None for any other decode; with coherent_drift
    (True or (max_rate, n_rates)) the fit is (dt_s, df_hz, rate_hz_per_s); a decode from a joint metric over
    2 or 3 symbols (coherent_nsym > 1) has MULTI_SYMBOL as a further, last entry.  With coherent_ap (needs ap
    and coherent) a result may carry both marks: its pattern and its fit.
    selection: "reference" or "topk".  subtract (True or a pass count in [2, 4]; not with snr): subtract-and-
    redecode with the retries above in every pass, and a last entry passes: per result the 1-based pass that
    appended it.  A decode from a residual has no fit entry (the stage call would fit it on the samples).
    osd (True, an order or (order, max_per_slot)): ordered-statistics decoding of what every other retry left
    failed, and a last entry orders: per result the configured order where that pass produced it, else None
    (such a result has no pattern)."""
    import torch
    from . import _lib
    from ._pipeline import decode_one
    from .ap import ap_index
    from .ft8_decode import selection_flags
    from .osd import osd_index, parse_option
    from .snr import snr_db_or_nan
    from .subtract import pass_of, passes_of, subtract_index
    flags = selection_flags(selection)
    subtract = passes_of(subtract)
    if subtract is not None and snr:
        raise NotImplementedError("no signal reports for a subtract decode")
    data, dtype, sample_rate = _read_raw(wave_path, verbose)
    _lib.require_gpu()
    dev = torch.device("cuda", _lib.device_index(device))
    if dtype == np.int16:   # raw PCM: the STFT kernel applies read_wave_file's float32 x / 32767
        x, code = torch.from_numpy(np.array(data, copy=True)).to(dev), _lib.FT8_I16
    else:
        h = data.astype(np.float32)
        h /= np.iinfo(dtype).max
        x, code = torch.from_numpy(h).to(dev), _lib.FT8_F32
    ap = None if ap is None else tuple(ap)
    results, reports, recs, *per_pass = decode_one(
        x, code, sample_rate, snr=snr, ap=ap, ap_max_hard_errors=ap_max_hard_errors, coherent=coherent,
        coherent_drift=coherent_drift, coherent_nsym=coherent_nsym, flags=flags, subtract=subtract,
        pass_counts=subtract is not None, coherent_ap=coherent_ap, osd=osd, osd_max_hard_errors=osd_max_hard_errors,
        **decode_kw)
    out = (results, snr_db_or_nan(reports) if snr else None,
           None if ap is None else [ap[ap_index(r) - 1] if ap_index(r) else None for r in recs])
    if coherent is not None:
        fits = _coherent_fits(x, code, sample_rate, recs, decode_kw, coherent_drift)
        out += ([None if subtract_index(r) else f for r, f in zip(recs, fits)],)
    if subtract is not None:
        out += ([pass_of(per_pass[0], i) for i in range(len(recs))],)
    if osd is not None and osd is not False:
        order = parse_option(osd)[0]
        out += ([order if osd_index(r) else None for r in recs],)
    return out


MULTI_SYMBOL = "multi-symbol"   # last entry of the fit of a decode from a multi-symbol set


def _coherent_fits(x, code, sample_rate, recs, decode_kw, drift=None):
    """(dt_s, df_hz) of every record the coherent pass rescued (the stage call on those candidates), None
    for the others; with the drift search (True or (max_rate, n_rates)) also the winning rate in Hz/s;
    MULTI_SYMBOL last for a record with pass_index bit 3."""
    from ._pipeline import make_plan
    from .coherent import DEFAULT_DRIFT, coherent_index, multisymbol_index
    from .ldpc_decoder import coherent_llr_batch
    fits = [None] * len(recs)
    idx = [i for i, r in enumerate(recs) if coherent_index(r)]
    if idx:
        bpt, sps = decode_kw.get("bins_per_tone", 2), decode_kw.get("steps_per_symbol", 2)
        plan = make_plan(int(x.shape[0]), sample_rate, bpt, sps, decode_kw.get("freq_min"), decode_kw.get("freq_max"),
                         decode_kw.get("time_min"), decode_kw.get("time_max"))
        cand = [(int(recs[i]["abs_time"]), int(recs[i]["abs_freq"])) for i in idx]
        if drift is None or drift is False:
            _, f = coherent_llr_batch(x, cand, [0] * len(idx), sample_rate, bpt, sps, plan.t_lo, plan.f_lo, code=code)
            for i, fi in zip(idx, f):
                fits[i] = (float(fi["dt_s"]), float(fi["df_hz"]))
        else:
            _, f, g = coherent_llr_batch(x, cand, [0] * len(idx), sample_rate, bpt, sps, plan.t_lo, plan.f_lo, code=code,
                                         drift=DEFAULT_DRIFT if drift is True else drift)
            for i, fi, gi in zip(idx, f, g):
                fits[i] = (float(fi["dt_s"]), float(fi["df_hz"]), float(gi["rate_hz_per_s"]))
        for i in idx:
            if multisymbol_index(recs[i]):
                fits[i] += (MULTI_SYMBOL,)
    return fits


def decode_ft8_from_wave(wave_path: str, freq_min: float = None, freq_max: float = None, time_min: float = None,
                         time_max: float = None, bins_per_tone: int = 2, steps_per_symbol: int = 2,
                         max_candidates: int = 20, min_score: float = 10, max_iterations: int = 20,
                         correction: bool = False, device=None, verbose: bool = False) -> list:
    """from_wave.py:71-178."""
    if correction:
        # from_wave.py:105-159 passes an FT8Waterfall as correct_frequency_drift's `params`, whose
        # default filling (frequency_correction.py:164-166) raises TypeError: the reference CLI's
        # correction path never decodes.  Same error here; the correction itself is available as
        # ft8_demodulator_amd.frequency_correction.correct_frequency_drift (GPU).
        raise TypeError("argument of type 'FT8Waterfall' is not iterable "
                        "(from_wave.py:152-158 passes a waterfall as correct_frequency_drift's params)")
    return _decode_file(wave_path, device=device, verbose=verbose, freq_min=freq_min, freq_max=freq_max,
                        time_min=time_min, time_max=time_max, bins_per_tone=bins_per_tone,
                        steps_per_symbol=steps_per_symbol, max_candidates=max_candidates, min_score=min_score,
                        max_iterations=max_iterations)[0]


def decode_ft8_from_wave_snr(wave_path: str, freq_min: float = None, freq_max: float = None, time_min: float = None,
                             time_max: float = None, bins_per_tone: int = 2, steps_per_symbol: int = 2,
                             max_candidates: int = 20, min_score: float = 10, max_iterations: int = 20,
                             device=None) -> tuple:
    """decode_ft8_from_wave with the signal report (build-defined): -> (results, snr_db), the same
    5-tuples and one SNR in 2500 Hz (dB, float) per result, measured on the device on the waterfall
    of the same decode (SlotDecoder.snr / ft8_snr_last)."""
    return _decode_file(wave_path, snr=True, device=device, freq_min=freq_min, freq_max=freq_max, time_min=time_min,
                        time_max=time_max, bins_per_tone=bins_per_tone, steps_per_symbol=steps_per_symbol,
                        max_candidates=max_candidates, min_score=min_score, max_iterations=max_iterations)[:2]


def decode_ft8_from_wave_ap(wave_path: str, ap, ap_max_hard_errors: int = None, freq_min: float = None,
                            freq_max: float = None, time_min: float = None, time_max: float = None,
                            bins_per_tone: int = 2, steps_per_symbol: int = 2, max_candidates: int = 20,
                            min_score: float = 10, max_iterations: int = 20, device=None) -> tuple:
    """decode_ft8_from_wave with a-priori decoding (build-defined): candidates BP fails on are retried
    with the patterns `ap` (ap.ap_hypothesis, e.g. ["CQ ? ?"]) -> (results, patterns, snr_db): the same
    5-tuples in candidate order, per result the pattern that rescued it (None for a plain decode), and
    its SNR in 2500 Hz as decode_ft8_from_wave_snr gives it."""
    results, snr_db, patterns = _decode_file(
        wave_path, snr=True, ap=ap, ap_max_hard_errors=ap_max_hard_errors, device=device, freq_min=freq_min,
        freq_max=freq_max, time_min=time_min, time_max=time_max, bins_per_tone=bins_per_tone,
        steps_per_symbol=steps_per_symbol, max_candidates=max_candidates, min_score=min_score,
        max_iterations=max_iterations)
    return results, patterns, snr_db


def _print_results(results, text: bool = False, snr=None, ap=None, coherent=None, passes=None, osd=None):
    """text: one extra `Message:` line per result, the payload unpacked to message text.  snr (one
    value per result): one extra `SNR:` line per result, dB in 2500 Hz.  ap (one pattern or None per
    result): one extra `AP: <pattern>` line for every a-priori decode.  coherent (one (dt_s, df_hz) or
    None per result): one extra `Coherent:` line for every decode from the coherent LLRs; a third entry
    (the drift search's rate, Hz/s) ends the line with `, drift +0.50 Hz/s`, and a last entry MULTI_SYMBOL
    with `, multi-symbol` after that.  passes (one 1-based pass per result): one extra `Pass: k` line for
    every decode a later pass of a subtract decode appended (k >= 2).  osd (one order or None per result): one
    extra `OSD: order k` line for every decode the ordered-statistics pass produced."""
    if not results:
        print("No FT8 messages decoded")
        return
    if text:
        from .message import text_of, unpack77
        texts = [text_of(t) if int(t["status"]) == 0 else f"(not decoded: status {int(t['status'])})"
                 for t in unpack77([bytes(r[0].payload) for r in results])]
    print("\nDecoded FT8 messages:")
    print("-" * 50)
    for k, (message, status, time_sec, freq_hz, score) in enumerate(results):
        print(f"Time: {time_sec:.2f} seconds")
        print(f"Frequency: {freq_hz:.1f} Hz")
        print(f"Score: {score:.1f}")
        if snr is not None:
            print(f"SNR: {snr[k]:.1f} dB")
        print(f"Payload: {message.payload.hex()}")
        if text:
            print(f"Message: {texts.pop(0)}")
        if ap is not None and ap[k] is not None:
            print(f"AP: {ap[k]}")
        if osd is not None and osd[k] is not None:
            print(f"OSD: order {osd[k]}")
        if coherent is not None and coherent[k] is not None:
            multi = coherent[k][-1] == MULTI_SYMBOL
            fit = coherent[k][:-1] if multi else coherent[k]
            drift = f", drift {fit[2]:+.2f} Hz/s" if len(fit) > 2 else ""
            print(f"Coherent: dt {fit[0] * 1e3:+.2f} ms, df {fit[1]:+.2f} Hz{drift}{', multi-symbol' if multi else ''}")
        if passes is not None and passes[k] > 1:
            print(f"Pass: {passes[k]}")
        print(f"CRC check: {status.crc_calculated}")
        print(f"LDPC errors: {status.ldpc_errors}")
        print("-" * 50)


def _decode_many(paths, correction, kw):
    """Several files (build-defined extension of the reference CLI): 16-bit PCM files of one sample
    rate and length are decoded as batches through the streaming path (stream.decode_wave_files);
    any other file -- and every file with --correction -- one at a time.  Results per file, in order."""
    from .stream import decode_wave_files
    out = [None] * len(paths)
    groups = {}
    for i, path in enumerate(paths):
        raw, dt, fs = _read_raw(path)
        if correction or dt != np.int16:
            out[i] = decode_ft8_from_wave(path, correction=correction, **kw)
        else:
            groups.setdefault((fs, raw.shape[0]), []).append(i)
    for idx in groups.values():
        res = decode_wave_files([paths[i] for i in idx], **kw)
        for i, r in zip(idx, res):
            out[i] = r
    return out


def _drift_arg(text: str):
    """--coherent-drift MAX[:N] -> (MAX Hz/s, N rates); N defaults to 9."""
    from .coherent import DEFAULT_DRIFT
    a, _, n = text.partition(":")
    return float(a), int(n) if n else DEFAULT_DRIFT[1]


def _osd_arg(text: str):
    """--osd ORDER[:N] -> (ORDER, N candidates per slot); N defaults to 32."""
    from .osd import DEFAULT_MAX_PER_SLOT
    a, _, n = text.partition(":")
    return int(a), int(n) if n else DEFAULT_MAX_PER_SLOT


def main(argv=None):
    """from_wave.py:180-229 (same flags).  Several wave files may be given (decoded as batches)."""
    parser = argparse.ArgumentParser(description="Decode FT8 signals from a wave file (MI355X GPU path)")
    parser.add_argument("wave_file", nargs="+", help="input wave file(s)")
    parser.add_argument("--freq-min", type=float, help="minimum frequency (Hz)")
    parser.add_argument("--freq-max", type=float, help="maximum frequency (Hz)")
    parser.add_argument("--time-min", type=float, help="minimum time (s)")
    parser.add_argument("--time-max", type=float, help="maximum time (s)")
    parser.add_argument("--bins-per-tone", type=int, default=2)
    parser.add_argument("--steps-per-symbol", type=int, default=2)
    parser.add_argument("--max-candidates", type=int, default=20)
    parser.add_argument("--min-score", type=float, default=10)
    parser.add_argument("--max-iterations", type=int, default=20)
    parser.add_argument("--correction", type=bool, default=False)
    parser.add_argument("--text", action="store_true", help="print each payload's message text as well")
    parser.add_argument("--snr", action="store_true", help="print each decode's SNR in 2500 Hz as well")
    parser.add_argument("--ap", action="append", metavar="PATTERN",
                        help='retry failed candidates with these message bits known, e.g. "CQ ? ?" or '
                             '"K1ABC ? ?" (repeatable, tried in order; an AP decode is marked with its pattern)')
    parser.add_argument("--ap-max-hard-errors", type=int, default=None,
                        help="most hard decisions of an AP decode that may contradict the received bits (default 36)")
    parser.add_argument("--coherent", nargs="?", type=int, const=-1, default=None, metavar="N",
                        help="demodulate the N best-scoring failed candidates again coherently from the samples "
                             "(default 32, 0: all; such a decode is marked with its fit's time and frequency offset)")
    parser.add_argument("--coherent-drift", nargs="?", type=_drift_arg, const=True, default=None, metavar="MAX[:N]",
                        help="with --coherent: also search N (odd, at most 33) linear frequency drift rates over "
                             "+-MAX Hz/s (at most 4) for each of those candidates (default 1.0:9; the decode's "
                             "mark then carries the rate)")
    parser.add_argument("--coherent-nsym", type=int, choices=(1, 2, 3), default=None, metavar="N",
                        help="with --coherent: also decode joint LLRs over 2 .. N (at most 3) adjacent symbols for "
                             "each of those candidates (default 1: off; such a decode's mark ends with multi-symbol)")
    parser.add_argument("--coherent-ap", action="store_true",
                        help="with --ap and --coherent: also retry those candidates with the --ap patterns on their "
                             "coherent LLRs (such a decode carries both marks)")
    parser.add_argument("--osd", nargs="?", type=_osd_arg, const=True, default=None, metavar="ORDER[:N]",
                        help="ordered-statistics decoding, order 0 to 2, of the first N candidates of the slot that "
                             "every other retry left failed (default 2:32, N = 0: all; such a decode is marked "
                             "with the order)")
    parser.add_argument("--osd-max-hard-errors", type=int, default=None,
                        help="most hard decisions of an OSD decode that may contradict the received bits (default 36)")
    parser.add_argument("--bp32", action="store_true",
                        help="run belief propagation in float32 (faster; decodes are no longer bit-identical to "
                             "the reference's float64 decoder)")
    parser.add_argument("--selection", choices=("reference", "topk"), default="reference",
                        help="candidate selection: the reference's, or the max-candidates highest scores")
    parser.add_argument("--ft4", action="store_true",
                        help="decode FT4 instead of FT8 (build-defined, interoperability with WSJT-X unverified; "
                             "not with --snr, --coherent, --subtract or --correction; FT4 scores are lower: "
                             "try --min-score 4 or --selection topk --min-score 0)")
    parser.add_argument("--subtract", nargs="?", type=int, const=2, default=None, metavar="PASSES",
                        help="subtract what each pass decodes and decode the residual again, PASSES passes in all "
                             "(2 to 4, default 2), with --ap / --coherent in every pass; a decode a later pass "
                             "added is marked with its pass (not with --snr)")
    args = parser.parse_args(argv)
    if args.subtract is not None:
        from .subtract import check_passes
        try:
            check_passes(args.subtract)
        except ValueError as e:
            parser.error(f"--subtract: {e}")
        if args.snr:
            parser.error("--subtract cannot report --snr (the waterfall left is the residual's)")
    coherent = None if args.coherent is None else (True if args.coherent < 0 else args.coherent)
    if args.ft4 and (args.snr or args.coherent is not None or args.subtract is not None or args.correction):
        parser.error("--ft4 takes none of --snr, --coherent, --subtract, --correction")
    if args.coherent_drift is not None and coherent is None:
        parser.error("--coherent-drift needs --coherent")
    if args.coherent_nsym is not None and coherent is None:
        parser.error("--coherent-nsym needs --coherent")
    if args.coherent_ap and (not args.ap or coherent is None):
        parser.error("--coherent-ap needs --ap and --coherent")
    if args.osd is not None:
        from .osd import check_max_hard_errors, parse_option
        try:
            parse_option(args.osd)
            if args.osd_max_hard_errors is not None:
                check_max_hard_errors(args.osd_max_hard_errors)
        except ValueError as e:
            parser.error(f"--osd: {e}")
    elif args.osd_max_hard_errors is not None:
        parser.error("--osd-max-hard-errors needs --osd")
    paths = args.wave_file
    for path in paths:
        if not os.path.exists(path):
            print(f"Error: File {path} does not exist")
            sys.exit(1)
    kw = dict(freq_min=args.freq_min, freq_max=args.freq_max, time_min=args.time_min, time_max=args.time_max,
              bins_per_tone=args.bins_per_tone, steps_per_symbol=args.steps_per_symbol,
              max_candidates=args.max_candidates, min_score=args.min_score, max_iterations=args.max_iterations)
    many = len(paths) > 1
    if (args.ap or args.snr or coherent is not None or args.subtract is not None or args.osd is not None
            or args.selection != "reference" or args.ft4 or args.bp32):
        # the report comes from the decode's own waterfall, an AP decode's mark from its own record:
        # one file at a time, each decoded once (lazily: a file is printed before the next is decoded)
        if args.correction:
            decode_ft8_from_wave(paths[0], correction=True)  # raises as without the flags
        if coherent is not None:
            kw = dict(kw, coherent=coherent)
        if args.coherent_drift is not None:
            kw = dict(kw, coherent_drift=args.coherent_drift)
        if args.coherent_nsym is not None:
            kw = dict(kw, coherent_nsym=args.coherent_nsym)
        if args.coherent_ap:
            kw = dict(kw, coherent_ap=True)
        if args.selection != "reference":
            kw = dict(kw, selection=args.selection)
        if args.ft4:
            kw = dict(kw, protocol="ft4")
        if args.bp32:
            kw = dict(kw, bp32=True)
        if args.subtract is not None:
            kw = dict(kw, subtract=args.subtract)
        if args.osd is not None:
            kw = dict(kw, osd=args.osd)
            if args.osd_max_hard_errors is not None:
                kw = dict(kw, osd_max_hard_errors=args.osd_max_hard_errors)
        decoded = (_decode_file(path, snr=args.snr, ap=args.ap, ap_max_hard_errors=args.ap_max_hard_errors, **kw)
                   for path in paths)
    elif many:
        decoded = ((results, None, None) for results in _decode_many(paths, args.correction, kw))
    else:
        decoded = [(decode_ft8_from_wave(paths[0], correction=args.correction, **kw), None, None)]
    per_file = []
    for path, (results, snr, patterns, *more) in zip(paths, decoded):
        if many:
            print(f"\n== {path}")
        fits = more.pop(0) if coherent is not None and more else None
        passes = more.pop(0) if args.subtract is not None and more else None
        orders = more.pop(0) if args.osd is not None and more else None
        _print_results(results, args.text, snr, patterns, fits, passes, orders)
        per_file.append(results)
    return per_file if many else per_file[0]


if __name__ == "__main__":
    main()
