"""Per-kernel timing on the GPU box (events on torch's current stream, which is the
stream the C-ABI launches on).  Usage: python tools/bench_kernels.py [cutout] [attn] [corr] [person] [grid] [gridmatch] [refine] [gridscroll] [gridstore] [cast] [novel] [merge] ..."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from planar_optical_flow_amd import ops, synth

def timeit(fn, iters=20, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters

which = set(sys.argv[1:]) or {"cutout", "attn", "corr"}
dev = "cuda"
if "cutout" in which:
    tab = ops.phi_table()
    for (B, T, fixed, P) in [(2048, 5, True, 56), (1024, 11, False, 56), (2048, 5, True, 48)]:
        sb = synth.make_batch(seed=3, B=B, T=T)
        scans = torch.from_numpy(sb.scans).to(dev)
        out = torch.empty((B, 450, T, P), dtype=torch.float32, device=dev)
        kw = dict(fixed=fixed, centered=True, window_width=1.0, window_depth=0.5, num_cutout_pts=P, padding_val=29.99, area_mode=True)
        ms = timeit(lambda: ops.cutout(scans, tab, out=out, **kw))
        byt = B * (T * 450 * 4 + 450 * T * P * 4)
        print("cutout B=%d T=%d fixed=%d P=%d: %.3f ms  %.0f GB/s  %.2f Msamples/s" % (B, T, fixed, P, ms, byt / ms / 1e6, B / ms / 1e3))
        ms = timeit(lambda: ops.cutout(scans, tab, out=out, exact_values=False, **kw))
        print("   float32 value path: %.3f ms  %.0f GB/s" % (ms, byt / ms / 1e6))
    # dense 3600-pt geometry (rows do not fit LDS)
    tab2 = ops.phi_table(np.radians(0.1), 3600)
    sb = synth.make_batch(seed=5, B=64, T=11, N=3600, angle_inc=np.radians(0.1))
    scans = torch.from_numpy(sb.scans).to(dev)
    out = torch.empty((64, 3600, 11, 56), dtype=torch.float32, device=dev)
    kw = dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5, num_cutout_pts=56, padding_val=29.99, area_mode=True)
    ms = timeit(lambda: ops.cutout(scans, tab2, out=out, **kw), iters=5)
    byt = 64 * (11 * 3600 * 4 + 3600 * 11 * 56 * 4)
    print("cutout dense3600 B=64 T=11: %.3f ms  %.0f GB/s" % (ms, byt / ms / 1e6))
if "attn" in which:
    for B in (16, 64, 256):
        N, E, F = 450, 128, 3584
        g = torch.Generator(device=dev).manual_seed(10)
        ex = torch.randn((B, N, E), device=dev, generator=g) * 0.3
        et = torch.randn((B, N, E), device=dev, generator=g) * 0.3
        x = torch.randn((B, N, F), device=dev, generator=g)
        t = torch.randn((B, N, F), device=dev, generator=g)
        out = torch.empty_like(x)
        per = 3 * N * F * 4 + 2 * N * E * 4 + 2 * N * 11 * 4
        ms = timeit(lambda: ops.spatial_attention(ex, et, x, t, 0.5, 11, out=out), iters=10)
        print("attn B=%d: %.3f ms  %.0f GB/s" % (B, ms, per * B / ms / 1e6))
if "corr" in which:
    for (B, C, n) in [(4096, 256, 57), (256, 256, 450)]:
        f1 = torch.randn((B, C, n), device=dev); f2 = torch.randn((B, C, n), device=dev)
        out = torch.empty((B, 11, n), device=dev)
        ms = timeit(lambda: ops.band_correlation(f1, f2, 3, 5, out=out), iters=10)
        byt = B * (2 * C * n * 4 + 11 * n * 4)
        print("corr B=%d C=%d n=%d: %.3f ms  %.0f GB/s  %.1f TFLOP/s" % (B, C, n, ms, byt / ms / 1e6, B * 2 * 11 * n * 3 * C / ms / 1e9))
if "bwd" in which:
    for (B, C, n) in [(4096, 256, 57)]:
        f1 = torch.randn((B, C, n), device=dev); f2 = torch.randn((B, C, n), device=dev)
        g = torch.randn((B, 11, n), device=dev)
        ms = timeit(lambda: ops.band_correlation_backward(f1, f2, g, 3, 5), iters=10)
        byt = B * (4 * C * n * 4 + 11 * n * 4)
        print("corr backward B=%d C=%d n=%d: %.3f ms  %.0f GB/s" % (B, C, n, ms, byt / ms / 1e6))
    for B in (64,):
        N, E, F = 450, 128, 3584
        gen = torch.Generator(device=dev).manual_seed(10)
        ex = torch.randn((B, N, E), device=dev, generator=gen) * 0.3
        et = torch.randn((B, N, E), device=dev, generator=gen) * 0.3
        x = torch.randn((B, N, F), device=dev, generator=gen)
        t = torch.randn((B, N, F), device=dev, generator=gen)
        out, band, prob = ops.spatial_attention(ex, et, x, t, 0.5, 11)
        go = torch.randn_like(out); gb = torch.randn_like(band)
        per = 4 * N * F * 4 + 4 * N * E * 4 + 3 * N * 11 * 4     # read g, tmpl; write dx, dtmpl; emb in/out
        for fused in (False, True):
            ms = timeit(lambda: ops.spatial_attention_backward(ex, et, t, prob, go, gb, 0.5, 11, fused=fused), iters=10)
            print("attn backward B=%d [%s]: %.3f ms  %.0f GB/s" % (B, "fused" if fused else "two-pass", ms,
                                                                    per * B / ms / 1e6))
if "polar" in which:
    B, Tn, N = 2048, 5, 450
    sb = synth.make_batch(seed=3, B=B, T=Tn)
    scans = torch.from_numpy(sb.scans).to(dev)
    out = torch.empty((B, Tn, 31, N), dtype=torch.float32, device=dev)
    ms = timeit(lambda: ops.polar_grid(scans, out=out))
    byt = B * Tn * N * 4 * 32
    print("polar grid B=%d T=%d: %.3f ms  %.0f GB/s" % (B, Tn, ms, byt / ms / 1e6))
if "f16" in which:
    for (B, C, n) in [(4096, 256, 57), (256, 256, 450)]:
        f1 = torch.randn((B, C, n), device=dev).half(); f2 = torch.randn((B, C, n), device=dev).half()
        out = torch.empty((B, 11, n), device=dev)
        ms = timeit(lambda: ops.band_correlation(f1, f2, 3, 5, out=out), iters=10)
        byt = B * (2 * C * n * 2 + 11 * n * 4)
        print("corr f16 B=%d C=%d n=%d: %.3f ms  %.0f GB/s" % (B, C, n, ms, byt / ms / 1e6))
    for B in (64, 256):
        N, E, F = 450, 128, 3584
        gen = torch.Generator(device=dev).manual_seed(10)
        ex = torch.randn((B, N, E), device=dev, generator=gen) * 0.3
        et = torch.randn((B, N, E), device=dev, generator=gen) * 0.3
        x = torch.randn((B, N, F), device=dev, generator=gen).half()
        t = torch.randn((B, N, F), device=dev, generator=gen).half()
        out = torch.empty_like(x)
        ms = timeit(lambda: ops.spatial_attention(ex, et, x, t, 0.5, 11, out=out), iters=10)
        per = 3 * N * F * 2 + 2 * N * E * 4 + 2 * N * 11 * 4
        print("attn f16 B=%d: %.3f ms  %.0f GB/s" % (B, ms, per * B / ms / 1e6))

if "boost" in which:
    # N4: boosted stumps.  Device rounds vs the NumPy restatement (which is already far faster than the
    # reference's interpreted per-sample loops) on a segment table of realistic size.
    import time
    from oracle import ref_numpy as R
    from planar_optical_flow_amd.src.depracted.model.adaboost_person_det import BoostedFeatureDetector
    rng = np.random.default_rng(0)
    N, D, K, ns = 50000, 12, 60, 200
    X = rng.normal(size=(N, D))
    Y = np.where(X @ rng.normal(size=D) + 1.5 * rng.normal(size=N) > 0, 1.0, -1.0)
    BoostedFeatureDetector(rng=np.random.default_rng(5)).adaboost(X[:1000], Y[:1000], 2, ns)      # warm-up
    det = BoostedFeatureDetector(rng=np.random.default_rng(1))
    t0 = time.time(); a, p = det.adaboost(X, Y, K, ns); torch.cuda.synchronize(); t1 = time.time()
    print("adaboost HIP   N=%d D=%d K=%d nSamples=%d: %.3f s (%.2f ms/round)" % (N, D, K, ns, t1 - t0, (t1 - t0) / K * 1e3))
    t0 = time.time(); a2, p2 = R.adaboost(X, Y, 6, ns, rng=np.random.default_rng(1)); t1 = time.time()
    print("adaboost NumPy restatement, 6 rounds: %.3f s (%.1f ms/round)" % (t1 - t0, (t1 - t0) / 6 * 1e3))
    assert np.array_equal(a[:6], a2) and np.array_equal(p[:6], p2)
    Xd = torch.from_numpy(X).cuda()
    ms = timeit(lambda: det.eval(Xd, a, p))
    print("eval (stump vote) N=%d K=%d: %.3f ms incl. D2H" % (N, K, ms))
    idx = torch.from_numpy(rng.integers(0, N, 2048).astype(np.int32)).cuda()
    Yd = torch.from_numpy(Y).cuda()
    for n in (200, 2048):
        ms = timeit(lambda: det._search(Xd, Yd, idx[:n].contiguous(), n))
        print("stump search n=%d D=%d: %.3f ms incl. D2H of the %d results" % (n, D, ms, 5 * D))

if "person" in which:
    # N5: per-person flow next to the centre NMS it follows, 1024 scans x 450 points.  Predictions as in
    # tests/golden/person_flow.npz (distinct sigmoid scores, regressions N(0, 0.3): about 105 detections per scan).
    B, N = 1024, 450
    rng = np.random.default_rng(1701)
    tab = ops.phi_table()
    scans = torch.from_numpy(synth.make_batch(seed=3, B=B, T=1).scans[:, 0].copy()).to(dev)
    logit = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.float64) / N * 8.0 - 4.0
    cls = torch.from_numpy(1.0 / (1.0 + np.exp(-logit))).to(dev)
    reg = torch.from_numpy(rng.normal(0, 0.3, (B, N, 2))).to(dev)
    flow = torch.from_numpy(rng.normal(0, 0.06, (B, N, 2)).astype(np.float32)).to(dev)
    ang = rng.uniform(-np.pi, np.pi, B)
    rot = torch.from_numpy(np.stack([np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)], 1).astype(np.float32)).to(dev)
    trans = torch.from_numpy(rng.uniform(40, 120, (B, 2))).to(dev)
    ftr = torch.from_numpy(rng.normal(0, 0.05, (B, 2))).to(dev)
    xy, dc, num, inst = ops.nms_predicted_center(scans, tab, cls, reg, 0.5)
    out = ops.person_flow_buffers(B, N, dev)
    # N6: the ego-motion fit on the same scans, flow and NMS results (the launch that sits between the two), plain
    # and with four Huber re-weightings
    ego_out = ops.ego_motion_buffers(B, N, dev)
    ego = lambda iters: ops.ego_motion(scans, tab, flow, instance_mask=inst, num_det=num, det_cls=dc, huber_delta=0.02,
                                       iters=iters, out=ego_out)
    # N8: the scan matcher on the same scans and NMS results; the previous scan is the same scene with range noise of
    # its own (the sensor stands still), every pair starts from rest.  One iteration, and the default 16 with the early
    # exit (the mean number of iterations run is printed)
    prev = torch.from_numpy(synth.make_batch(seed=3, B=B, T=2).scans[:, 1].copy()).to(dev)
    sm_out = ops.scan_match_buffers(B, N, dev)
    match = lambda iters: ops.scan_match(prev, scans, tab, instance_mask=inst, num_det=num, det_cls=dc, iters=iters,
                                         out=sm_out)
    # N9: the keyframe matcher on the same inputs: `prev` seeds the keyframe of every sensor, then every timed call
    # matches `scans` against it from rest (key_rel is zeroed in front of the launch: one memset node, timed on its own
    # too); the sensor stands still, so no keyframe is replaced and the state stays what it was
    kf_state, kf_out = ops.keyframe_buffers(B, N, dev), ops.keyframe_match_buffers(B, N, dev)
    ops.keyframe_match(prev, tab, kf_state)

    def keyframe(iters):
        kf_state.key_rel.zero_()
        ops.keyframe_match(scans, tab, kf_state, instance_mask=inst, num_det=num, det_cls=dc, iters=iters, out=kf_out)
    # N10: the keyframe map on the same inputs, with one slot and with sixteen: `prev` seeds slot 0 of every sensor, the
    # rest as N9's row.  The sensor stands still, so no step leaves its keyframe and the slot search never runs
    km_state = {K: ops.keyframe_map_buffers(B, N, K, dev) for K in (1, 16)}
    km_out = ops.keyframe_map_match_buffers(B, N, dev)
    for K in km_state:
        ops.keyframe_map_match(prev, tab, km_state[K])

    def keyframe_map(K, iters):
        km_state[K].key_rel.zero_()
        ops.keyframe_map_match(scans, tab, km_state[K], instance_mask=inst, num_det=num, det_cls=dc, iters=iters,
                               out=km_out)
    # N7: the track update on the per-person result of these scans.  The same detections every call: after the first
    # one every candidate (score >= 0.5, about half the detections) is matched with its track -- the steady state
    ops.person_flow(flow, tab, inst, num, xy, dc, rot, trans, ftr, 0.5, out=out)
    tracks = {M: ops.track_buffers(B, M, N, dev) for M in (64, 256)}
    track = lambda M: ops.track_update(out.det_xy_world, out.det_flow, out.det_valid, num, inst, tracks[M])
    # N15: the map check of those tracks, next to the track update on the same state.  The grid's outputs are those of
    # the second of two updates of a 128 x 128 grid of 0.25 m with the same scan (every burned-in point finds its own
    # hit), so the same rows add to the same slots every call and the sums halve whenever they pass the cap: the steady
    # state of a long sequence
    tm_grid = ops.grid_map_reset(ops.grid_map_state(B, 128, 128, dev), trans - 16.0)
    for _ in range(2):
        tm_seen = ops.grid_map_update(scans, tab, rot, trans, tm_grid, res=0.25, instance_mask=inst, num_det=num, det_cls=dc)
    tm_state = {M: ops.track_map_state(B, M, dev) for M in tracks}
    tm_out = {M: ops.track_map_buffers(B, M, N, dev) for M in tracks}
    tmap = lambda M: ops.track_map(tracks[M], tm_seen, inst, num, tm_state[M], out=tm_out[M])
    # N11: person motion on the same scans, NMS results and pose.  The same scan every call: after the first one every
    # candidate finds its own centroid of the call before -- the steady state, both pairwise searches run in full
    pm_state, pm_out = ops.person_motion_state(B, N, dev), ops.person_motion_buffers(B, N, dev)
    motion = lambda: ops.person_motion(scans, tab, inst, num, xy, dc, rot, trans, pm_state, out=pm_out)
    for rep in range(3):                                   # alternating, to see the spread
        ms_nms = timeit(lambda: ops.nms_predicted_center(scans, tab, cls, reg, 0.5), iters=50)
        ms_pf = timeit(lambda: ops.person_flow(flow, tab, inst, num, xy, dc, rot, trans, ftr, 0.5, out=out), iters=50)
        ms_e0, ms_e4 = timeit(lambda: ego(0), iters=50), timeit(lambda: ego(4), iters=50)
        print("B=%d N=%d (%.0f detections per scan): centre NMS %.3f ms, person flow %.3f ms, ego_motion %.3f ms "
              "(iters=0) %.3f ms (iters=4)" % (B, N, num.float().mean().item(), ms_nms, ms_pf, ms_e0, ms_e4))
        ms_m1, ms_m16 = timeit(lambda: match(1), iters=50), timeit(lambda: match(16), iters=50)
        print("   scan_match %.3f ms (iters=1) %.3f ms (iters=16: %.1f run per pair, %.0f points matched, %d of %d pairs ok)"
              % (ms_m1, ms_m16, sm_out.iters_used.float().mean().item(), sm_out.count.float().mean().item(),
                 int(sm_out.ok.sum().item()), B))
        ms_k1, ms_k16 = timeit(lambda: keyframe(1), iters=50), timeit(lambda: keyframe(16), iters=50)
        ms_z = timeit(lambda: kf_state.key_rel.zero_(), iters=50)
        print("   keyframe_match %.3f ms (iters=1) %.3f ms (iters=16: %.1f run per sensor, %.0f points matched, %d of %d "
              "ok, %d keyframes replaced), both with the %.3f ms memset of key_rel in front"
              % (ms_k1, ms_k16, kf_out.iters_used.float().mean().item(), kf_out.count.float().mean().item(),
                 int(kf_out.ok.sum().item()), B, int(kf_out.key_replaced.sum().item()), ms_z))
        for K in km_state:
            ms_k1, ms_k16 = timeit(lambda: keyframe_map(K, 1), iters=50), timeit(lambda: keyframe_map(K, 16), iters=50)
            print("   keyframe_map_match keys=%d %.3f ms (iters=1) %.3f ms (iters=16: %.1f run per sensor, %.0f points "
                  "matched, %d of %d ok, %d keyframes stored, %d switches), both with the memset of key_rel in front"
                  % (K, ms_k1, ms_k16, km_out.iters_used.float().mean().item(), km_out.count.float().mean().item(),
                     int(km_out.ok.sum().item()), B, int(km_out.key_replaced.sum().item()),
                     int(km_out.key_switched.sum().item())))
        ms_pm = timeit(motion, iters=50)
        print("   person_motion %.3f ms next to person flow %.3f ms (%.0f candidates per scan, %.0f paired)"
              % (ms_pm, ms_pf, pm_state.prev_cand.sum().item() / B, (pm_out.det_prev >= 0).sum().item() / B))
        ms_t = {M: timeit(lambda: track(M), iters=50) for M in tracks}
        print("   track_update (%.0f candidates per scan): %s" % (out.det_valid.sum().item() / B, ", ".join(
            "max_tracks %d: %.3f ms, %.0f live tracks per sensor" % (M, ms_t[M], (tracks[M].track_id > 0).sum().item() / B)
            for M in tracks)))
        ms_tm = {M: timeit(lambda: tmap(M), iters=50) for M in tracks}
        print("   track_map next to it: %s" % ", ".join(
            "max_tracks %d: %.3f ms (track_update %.3f ms), %.0f slots with evidence per sensor, classes %s"
            % (M, ms_tm[M], ms_t[M], (tm_state[M].ev_scans > 0).sum().item() / B,
               tm_out[M].class_count.sum(dim=0).tolist()) for M in tracks))

if which & {"grid", "gridmatch", "refine", "gridscroll", "gridstore", "cast", "novel", "merge"}:
    # N12: the occupancy grid map, 450 beams into 512 x 512 cells of 0.1 m per sensor, for 1024, 8 and 1 sensors, next
    # to person_motion on the same scans, NMS results and pose (alternating, three repeats of 50 launches).  The same
    # scan every call, with lo / hi at the int16 limits so that no cell saturates inside the run and every launch
    # stores what a first scan would.  Bytes: 2 * H * W * 2 per sensor is the bound of a launch that loads and stores
    # the whole grid; `changed` counts the 16-byte runs one launch really stored, `near` the share of tiles that are
    # not left at once (nearest point within max_range, or inside the box of the endpoints).
    # gridmatch: N13 next to it on the same scans, NMS results, pose and grid (the grid as two updates left it, a copy
    # so that the search reads the same cells every call), defaults: 9 rotations x 81 translations.  The pose starts
    # off by (0.23, -0.17) m and 0.02 rad; a moved pose stays moved, so from the second launch on the search starts
    # where the first one ended (the work of a launch does not depend on it).  Gathers: 9 * 81 * votes int16.
    # refine: N19 next to grid_match and scan_match, alternating, on the same scans, NMS results and grid (a copy, as two
    # updates left it, cloned before any other sub-command updates it again: every burned-in cell holds 34, above the
    # cap of 32, every freed cell -16).  Every launch starts from the map's pose
    # moved by (0.03, -0.02) m and 0.004 rad: three small copies on the stream put pose, rot and trans back in front
    # of it, timed on their own as well.  scan_match: the previous scan is the same scene with range noise of its own,
    # every pair from rest, defaults.  Gathers: 4 * (iters_used + 1) * count int16.
    # gridscroll: N14 next to grid_map_update on a copy of the same grid, two cases.  `stays`: the sensor in the middle
    # of its grid as it stands, what every step pays (two launches that leave at once).  `scrolls`: every sensor scrolls
    # in every call -- the position alternates between tile 7 of 8 and, seen from the grid so scrolled, tile 1, on both
    # axes, so the calls shift by +3 and -3 tiles and the offset alternates between 3 and 0.  A scroll writes the
    # grid twice and reads it once and the (5/8)^2 of it that stay: the bound of 4 * H * W * 2 bytes per sensor is
    # what a one-tile shift comes near.  Both cases form their position with one small add on the stream.
    # cast: N16 next to grid_map_update, alternating, on a copy of the grid as two updates left it (every endpoint that
    # is nobody's burned in twice, every cell in front of it freed twice: a map that knows the scene), the same scans,
    # NMS results and pose.  Cell reads: the sum of exp_steps, int16 gathers of one lane each.
    # novel: N17 next to grid_cast and person_motion, alternating, on the cast sub-command's own map.  That map holds the
    # scan itself, so the scan cast through it has no NOVEL point; the stage is therefore timed on two sets of classes:
    # `walkers`, the cast of the same scans with every sixth run of 10 beams pulled to 70 % of its range (somebody in
    # front of the wall, in space the map saw empty), and `all`, every byte NOVEL -- the most members a scan can have.
    # merge: N18 next to novel_segments and person_motion, alternating, on the novel sub-command's `walkers` scans and
    # classes: the segments of that cast merged with the NMS record.  Two legs: `nms`, the scores as the NMS gave them
    # (segments over confident detections are absorbed), and `all kept`, A's scores lowered to 0 so that every segment
    # with a point is appended -- the most rows the stage copies.
    N, H, W, RES = 450, 512, 512, 0.1
    rng = np.random.default_rng(1701)
    tab = ops.phi_table()
    for B in (1024, 8, 1):
        scans = torch.from_numpy(synth.make_batch(seed=3, B=B, T=1).scans[:, 0].copy()).to(dev)
        logit = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.float64) / N * 8.0 - 4.0
        cls = torch.from_numpy(1.0 / (1.0 + np.exp(-logit))).to(dev)
        reg = torch.from_numpy(rng.normal(0, 0.3, (B, N, 2))).to(dev)
        ang = rng.uniform(-np.pi, np.pi, B)
        rot = torch.from_numpy(np.stack([np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)], 1).astype(np.float32)).to(dev)
        trans = torch.from_numpy(rng.uniform(40, 120, (B, 2))).to(dev)
        xy, dc, num, inst = ops.nms_predicted_center(scans, tab, cls, reg, 0.5)
        pm_state, pm_out = ops.person_motion_state(B, N, dev), ops.person_motion_buffers(B, N, dev)
        motion = lambda: ops.person_motion(scans, tab, inst, num, xy, dc, rot, trans, pm_state, out=pm_out)
        gm_state, gm_out = ops.grid_map_state(B, H, W, dev), ops.grid_map_buffers(B, N, dev)
        ops.grid_map_reset(gm_state, trans - 0.5 * RES * torch.tensor([W, H], dtype=torch.float64, device=dev))
        grid = lambda: ops.grid_map_update(scans, tab, rot, trans, gm_state, res=RES, instance_mask=inst, num_det=num,
                                           det_cls=dc, lo=-32767, hi=32767, out=gm_out)
        grid()
        before = gm_state.grid.clone()
        grid()
        runs = int((gm_state.grid != before).view(B, H, W // 8, 8).any(dim=3).sum().item())
        touched = (gm_state.grid != 0).view(B, H // 64, 64, W // 64, 64).any(dim=4).any(dim=2).float().mean().item()
        two_updates = gm_state.grid.clone()                    # the grid as these two updates left it, for `refine`
        del before
        if "gridmatch" in which:
            sg_state = ops.GridMapState(gm_state.grid.clone(), gm_state.origin.clone())
            sg_out, sg_table = ops.grid_match_buffers(B, device=dev), ops.grid_match_table(device=dev)
            off = torch.tensor([0.23, -0.17, 0.02], dtype=torch.float64, device=dev)
            pose = torch.cat([trans, torch.from_numpy(ang).to(dev)[:, None]], dim=1) + off
            sg_rot = torch.stack([pose[:, 2].cos(), -pose[:, 2].sin(), pose[:, 2].sin(), pose[:, 2].cos()], 1).float().contiguous()
            sg_trans = pose[:, :2].contiguous()
            match = lambda: ops.grid_match(scans, tab, sg_rot, sg_trans, pose, sg_state, res=RES, table=sg_table,
                                           instance_mask=inst, num_det=num, det_cls=dc, out=sg_out)
            match()
            first = (sg_out.moved.sum().item(), sg_out.ok.sum().item())
            for rep in range(3):
                ms_g, ms_m = timeit(grid, iters=50), timeit(match, iters=50)
                print("gridmatch B=%d N=%d %dx%d at %.2f m: grid_match %.3f ms (%.2f us per sensor) next to grid_map_update "
                      "%.3f ms; %.0f voting points per scan, %.1f M int16 gathers per launch; first launch ok %d, moved %d "
                      "of %d" % (B, N, H, W, RES, ms_m, ms_m / B * 1e3, ms_g, sg_out.votes.sum().item() / B,
                                 9 * 81 * sg_out.votes.sum().item() / 1e6, first[1], first[0], B))
            del sg_state
        if "refine" in which:
            gr_state = ops.GridMapState(two_updates, gm_state.origin.clone())
            gr_out, sg_out = ops.grid_refine_buffers(B, dev), ops.grid_match_buffers(B, device=dev)
            sg_table, sm_out = ops.grid_match_table(device=dev), ops.scan_match_buffers(B, N, dev)
            prev = torch.from_numpy(synth.make_batch(seed=3, B=B, T=2).scans[:, 1].copy()).to(dev)
            off = torch.tensor([0.03, -0.02, 0.004], dtype=torch.float64, device=dev)
            pose0 = torch.cat([trans, torch.from_numpy(ang).to(dev)[:, None]], dim=1) + off
            rot0 = torch.stack([pose0[:, 2].cos(), -pose0[:, 2].sin(), pose0[:, 2].sin(), pose0[:, 2].cos()], 1).float().contiguous()
            trans0 = pose0[:, :2].contiguous()
            pose, gr_rot, gr_trans = pose0.clone(), rot0.clone(), trans0.clone()

            def put_back():
                pose.copy_(pose0); gr_rot.copy_(rot0); gr_trans.copy_(trans0)

            def refine():
                put_back()
                ops.grid_refine(scans, tab, gr_rot, gr_trans, pose, gr_state, res=RES, instance_mask=inst, num_det=num,
                                det_cls=dc, out=gr_out)

            def whole_cell():
                put_back()
                ops.grid_match(scans, tab, gr_rot, gr_trans, pose, gr_state, res=RES, table=sg_table, instance_mask=inst,
                               num_det=num, det_cls=dc, out=sg_out)

            pair = lambda: ops.scan_match(prev, scans, tab, instance_mask=inst, num_det=num, det_cls=dc, out=sm_out)
            refine()
            left = (pose - (pose0 - off))[gr_out.moved.bool()].abs().max(dim=0).values.tolist() if gr_out.moved.any() else []
            for rep in range(3):
                ms_r, ms_m, ms_s, ms_c = (timeit(f, iters=50) for f in (refine, whole_cell, pair, put_back))
                print("refine B=%d N=%d %dx%d at %.2f m: grid_refine %.3f ms (%.2f us per sensor) next to grid_match %.3f ms "
                      "and scan_match %.3f ms (%.1f iterations per pair); the three copies in front of the first two "
                      "%.3f ms; %.0f voting points per scan, %.0f inside, %.2f updates per sensor, %.2f M int16 gathers per "
                      "launch; ok %d, moved %d of %d, left of the offset %s"
                      % (B, N, H, W, RES, ms_r, ms_r / B * 1e3, ms_m, ms_s, sm_out.iters_used.float().mean().item(), ms_c,
                         gr_out.votes.sum().item() / B, gr_out.count.sum().item() / B,
                         gr_out.iters_used.float().mean().item(),
                         4 * ((gr_out.iters_used + 1) * gr_out.count).sum().item() / 1e6, gr_out.ok.sum().item(),
                         gr_out.moved.sum().item(), B, ["%.4f" % v for v in left]))
            del gr_state
        if "gridscroll" in which:
            gs_state = ops.GridMapState(gm_state.grid.clone(), gm_state.origin.clone())
            gs_scroll = ops.grid_scroll_reset(ops.grid_scroll_state(B, H, W, dev), gs_state)
            gs_out = ops.grid_scroll_buffers(B, dev)
            # positions relative to the origin as it then stands: the middle; tile 7 (-> +3); tile 1 (-> -3)
            at = lambda cx, cy: torch.tensor([(cx + 0.5) * RES, (cy + 0.5) * RES], dtype=torch.float64, device=dev)
            middle, up, down = at(W // 2, H // 2), at(W - 64, H - 64), at(64, 64)
            stays = lambda: ops.grid_scroll(gs_state.origin + middle, gs_state, gs_scroll, res=RES, out=gs_out)
            flip = [0]

            def scrolls():
                flip[0] ^= 1
                ops.grid_scroll(gs_state.origin + (up if flip[0] else down), gs_state, gs_scroll, res=RES, out=gs_out)

            scrolls()
            assert bool(gs_out.scrolled.all())
            scrolls()
            for rep in range(3):
                ms_g, ms_0, ms_1 = timeit(grid, iters=50), timeit(stays, iters=50), timeit(scrolls, iters=50)
                assert bool(gs_out.scrolled.all()) and int(gs_scroll.offset.abs().max()) <= 3
                moved = B * 4 * H * W * 2
                print("gridscroll B=%d %dx%d at %.2f m: no sensor scrolls %.3f ms, every sensor scrolls %.3f ms (%.2f us per "
                      "sensor, %.0f GB/s against the bound of 4*H*W*2 bytes per sensor) next to "
                      "grid_map_update %.3f ms" % (B, H, W, RES, ms_0, ms_1, ms_1 / B * 1e3, moved / ms_1 / 1e6, ms_g))
            del gs_state, gs_scroll
        if "gridstore" in which:
            # N20 next to N14 on copies of the same grid with every unknown cell set to 1, so that every tile that
            # leaves is stored: 64 slots per sensor, the same two cases and positions as gridscroll.  What the first
            # scroll brings in is unknown and would take no slot on its way out, so it is set to 1 as well: from the
            # second call on every scrolling call stores the 39 tiles that leave and restores the 39 that come back.
            full = torch.where(gm_state.grid == 0, torch.ones_like(gm_state.grid), gm_state.grid)
            at = lambda cx, cy: torch.tensor([(cx + 0.5) * RES, (cy + 0.5) * RES], dtype=torch.float64, device=dev)
            middle, up, down = at(W // 2, H // 2), at(W - 64, H - 64), at(64, 64)
            legs = {}
            for name in ("grid_scroll", "grid_scroll_store"):
                st = ops.GridMapState(full.clone(), gm_state.origin.clone())
                sc = ops.grid_scroll_reset(ops.grid_scroll_state(B, H, W, dev), st)
                if name == "grid_scroll":
                    out = ops.grid_scroll_buffers(B, dev)
                    call = lambda pos, st=st, sc=sc, out=out: ops.grid_scroll(st.origin + pos, st, sc, res=RES, out=out)
                else:
                    out, tiles = ops.grid_scroll_store_buffers(B, dev), ops.grid_store_state(B, H, W, 64, dev)
                    call = lambda pos, st=st, sc=sc, out=out, tiles=tiles: ops.grid_scroll_store(
                        st.origin + pos, st, sc, tiles, res=RES, out=out)
                legs[name] = (call, out, [0], st)

            def stays(name):
                return lambda: legs[name][0](middle)

            def scrolls(name):
                def f():
                    legs[name][2][0] ^= 1
                    legs[name][0](up if legs[name][2][0] else down)
                return f

            for name in legs:
                scrolls(name)()
                legs[name][3].grid.masked_fill_(legs[name][3].grid == 0, 1)
                scrolls(name)()
                assert bool(legs[name][1].scrolled.all())
            for rep in range(3):
                ms = {(name, case): timeit(f(name), iters=50) for name in legs for case, f in (("stays", stays), ("scrolls", scrolls))}
                counts = legs["grid_scroll_store"][1].counts
                assert bool((counts[:, 2:] == 0).all()) and bool((counts[:, 0] == counts[:, 1]).all())
                moved = int(counts[0, 1])
                plain, stored = B * 4 * H * W * 2, B * (4 * H * W * 2 + 2 * 2 * moved * 8192)
                print("gridstore B=%d %dx%d at %.2f m, 64 slots: no sensor scrolls %.3f ms (grid_scroll %.3f ms, +%.4f ms); every "
                      "sensor scrolls, %d tiles stored and %d restored per sensor %.3f ms (%.2f us per sensor, %.0f GB/s against "
                      "4*H*W*2 + 2*2*%d*8192 bytes per sensor) next to grid_scroll %.3f ms (%.0f GB/s against 4*H*W*2)"
                      % (B, H, W, RES, ms["grid_scroll_store", "stays"], ms["grid_scroll", "stays"],
                         ms["grid_scroll_store", "stays"] - ms["grid_scroll", "stays"], moved, int(counts[0, 0]),
                         ms["grid_scroll_store", "scrolls"], ms["grid_scroll_store", "scrolls"] / B * 1e3,
                         stored / ms["grid_scroll_store", "scrolls"] / 1e6, moved, ms["grid_scroll", "scrolls"],
                         plain / ms["grid_scroll", "scrolls"] / 1e6))
            del legs, full
        if "cast" in which:
            gc_state = ops.GridMapState(gm_state.grid.clone(), gm_state.origin.clone())
            gc_out = ops.grid_cast_buffers(B, N, dev)
            cast = lambda: ops.grid_cast(scans, tab, rot, trans, gc_state, res=RES, instance_mask=inst, num_det=num,
                                         det_cls=dc, out=gc_out)
            cast()
            steps = gc_out.exp_steps.sum().item()
            for rep in range(3):
                ms_g, ms_c = timeit(grid, iters=50), timeit(cast, iters=50)
                print("cast B=%d N=%d %dx%d at %.2f m: grid_cast %.3f ms (%.2f us per sensor) next to grid_map_update %.3f ms; "
                      "%.1f M cell reads per launch (%.0f per beam, the longest walk %d), %.1f G cells/s; beams per state "
                      "%s, points per class %s"
                      % (B, N, H, W, RES, ms_c, ms_c / B * 1e3, ms_g, steps / 1e6, steps / (B * N),
                         gc_out.exp_steps.max().item(), steps / ms_c / 1e6,
                         torch.bincount(gc_out.exp_state.flatten().long(), minlength=5).tolist(),
                         gc_out.class_count.sum(dim=0).tolist()))
            del gc_state
        if "novel" in which:
            ns_state = ops.GridMapState(gm_state.grid.clone(), gm_state.origin.clone())
            ns_cast_out, ns_out = ops.grid_cast_buffers(B, N, dev), ops.novel_segments_buffers(B, N, dev)
            near = scans.clone()
            pulled = (torch.arange(N, device=dev) // 10) % 6 == 2
            near[:, pulled] *= 0.7
            ns_cast = lambda: ops.grid_cast(near, tab, rot, trans, ns_state, res=RES, instance_mask=inst, num_det=num,
                                            det_cls=dc, out=ns_cast_out)
            ns_cast()
            walkers = ns_cast_out.point_class.clone()
            every = torch.full_like(walkers, 2)
            for name, classes in (("walkers", walkers), ("all", every)):
                novel = lambda: ops.novel_segments(near, tab, classes, instance_mask=inst, num_det=num, det_cls=dc,
                                                   out=ns_out)
                novel()
                for rep in range(3):
                    ms_c, ms_pm, ms_n = timeit(ns_cast, iters=50), timeit(motion, iters=50), timeit(novel, iters=50)
                    print("novel B=%d N=%d classes=%s: novel_segments %.3f ms (%.2f us per sensor) next to grid_cast %.3f ms "
                          "and person_motion %.3f ms; per scan %.0f members, %.1f segments, %.1f kept, %.1f few, %.1f wide, "
                          "%.1f points known to the NMS"
                          % (B, N, name, ms_n, ms_n / B * 1e3, ms_c, ms_pm, (classes == 2).sum().item() / B,
                             ns_out.seg_count[:, 0].sum().item() / B, ns_out.num_det.sum().item() / B,
                             ns_out.seg_count[:, 1].sum().item() / B, ns_out.seg_count[:, 2].sum().item() / B,
                             ns_out.det_known.sum().item() / B))
            del ns_state
        if "merge" in which:
            mg_state = ops.GridMapState(gm_state.grid.clone(), gm_state.origin.clone())
            mg_cast_out = ops.grid_cast_buffers(B, N, dev)
            ns_out, mg_out = ops.novel_segments_buffers(B, N, dev), ops.merge_detections_buffers(B, N, dev)
            near = scans.clone()
            near[:, (torch.arange(N, device=dev) // 10) % 6 == 2] *= 0.7
            ops.grid_cast(near, tab, rot, trans, mg_state, res=RES, instance_mask=inst, num_det=num, det_cls=dc,
                          out=mg_cast_out)
            walkers = mg_cast_out.point_class
            novel = lambda: ops.novel_segments(near, tab, walkers, instance_mask=inst, num_det=num, det_cls=dc, out=ns_out)
            novel()
            for name, scores in (("nms", dc), ("all kept", torch.zeros_like(dc))):
                merge = lambda: ops.merge_detections(*ns_out[:4], instance_mask=inst, num_det=num, det_xy=xy,
                                                     det_cls=scores, out=mg_out)
                merge()
                for rep in range(3):
                    ms_n, ms_pm, ms_m = timeit(novel, iters=50), timeit(motion, iters=50), timeit(merge, iters=50)
                    mc = mg_out.merge_count.sum(dim=0).tolist()
                    print("merge B=%d N=%d scores=%s: merge_detections %.3f ms (%.2f us per sensor) next to novel_segments "
                          "%.3f ms and person_motion %.3f ms; per scan %.1f NMS rows, %.1f segments: %.1f appended, %.1f "
                          "absorbed, %.1f dropped; %.1f points changed rows"
                          % (B, N, name, ms_m, ms_m / B * 1e3, ms_n, ms_pm, mc[0] / B, ns_out.num_det.sum().item() / B,
                             mc[1] / B, mc[2] / B, mc[3] / B, (mg_out.instance_mask != inst).sum().item() / B))
            del mg_state
        for rep in range(3 if "grid" in which else 0):
            ms_g, ms_pm = timeit(grid, iters=50), timeit(motion, iters=50)
            bound = B * 2 * H * W * 2
            print("grid B=%d N=%d %dx%d at %.2f m: grid_map_update %.3f ms (%.2f us per sensor) next to person_motion %.3f ms; "
                  "%.0f GB/s against the bound of 2*H*W*2 bytes per sensor, %.1f MB really stored (%d changed 16-byte runs), "
                  "%.2f of the tiles hold a known cell; %.0f marked points per scan"
                  % (B, N, H, W, RES, ms_g, ms_g / B * 1e3, ms_pm, bound / ms_g / 1e6, runs * 16 / 1e6, runs, touched,
                     gm_out.point_mark.sum().item() / B))
        del gm_state
