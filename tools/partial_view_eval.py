"""Registration on self-occluded views: `python tools/partial_view_eval.py [--json PATH]`.

shapenet_eval.evaluate with --features fpfh on the ten clouds of tests/golden/real_clouds10.npz and the 32 synthetic clouds of
tools/fpfh_bench.py (synth.make_cloud(c, 15000)[:10000]), one pose per cloud, for --registration {ransac, fgr, ransac_fm} and
sc2 (on the k-NN lists at k = 1 and 5 -- a list above 32 768 pairs is refused and recorded as such --, its
defaults, max_corr 2 voxels) x partial view {off, on}: with the option on, the posed copy of every pair is what one virtual
depth camera sees of it (cs_render_views, the defaults of shapenet_eval.Config), the model stays whole.  Per run: median and
largest RRE (degrees) and RTE of the estimator's pose (the *_ransac columns; FPFH runs without the symmetry hypotheses), the share of pairs within 15
degrees, and the mean visible share.  Then one line with --icp-iters 30 (point-to-point, the default distance) behind the
estimator with the largest share within 15 degrees on the partial views (ties: the smaller median RRE).
ppf: point-pair-feature voting, which reads no descriptors (max_corr 2 voxels is its verification radius, the
scene is oriented towards its camera on the partial views; a model above 4 096 voxels is refused and recorded as such),
ppf_v06: the same at twice the voxel size (0.06, max_corr 2 of those voxels), where every model fits, and ppf_icp: the same with --icp-iters point-to-point updates
behind it.  --only NAME,NAME runs those rows alone and merges them into the JSON that exists, so that the rows measured
earlier keep their numbers.
No outcome was fixed in advance.  One seed, one pose per cloud, 42 pairs: seeds move every figure, and no real scan is
measured.  Prints one JSON line; default PATH profiles/partial_view_eval.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, shapenet_eval as SE, synth  # noqa: E402

ESTIMATORS = ("ransac", "fgr", "ransac_fm")
# run name -> Config options: the estimators above at their defaults, and sc2 on the 1-NN and on the 5-NN lists
RUNS = dict([(e, dict(registration=e)) for e in ESTIMATORS] +
            [("sc2_k%d" % k, dict(registration="sc2", k_nn=k, max_corr=2 * SE.Config.voxel_size)) for k in (1, 5)] +
            [("ppf", dict(registration="ppf", max_corr=2 * SE.Config.voxel_size)),
             ("ppf_v06", dict(registration="ppf", voxel_size=2 * SE.Config.voxel_size, max_corr=4 * SE.Config.voxel_size))])
PPF_ICP = "ppf_icp"       # the ppf row again with the ICP behind it (reported from the *_icp columns)


def clouds():
    z = np.load(os.path.join(ROOT, "tests", "golden", "real_clouds10.npz"))
    real = [c.astype(np.float32) for c in z["clouds"]]
    return real, [synth.make_cloud(c, 15000)[:10000] for c in range(32)]


def report(results, tag, n_real):
    rre = np.degrees(np.asarray([r["rre_" + tag] for r in results]))
    rte = np.asarray([r["rte_" + tag] for r in results])
    out = {"rre_deg_median": round(float(np.median(rre)), 3), "rre_deg_max": round(float(rre.max()), 3),
           "rte_median": round(float(np.median(rte)), 4), "rte_max": round(float(rte.max()), 4),
           "within_15deg": round(float(np.mean(rre <= 15.0)), 4),
           "within_15deg_real": round(float(np.mean(rre[:n_real] <= 15.0)), 4),
           "within_15deg_synthetic": round(float(np.mean(rre[n_real:] <= 15.0)), 4)}
    if "visible_share" in results[0]:
        out["visible_share_mean"] = round(float(np.mean([r["visible_share"] for r in results])), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "partial_view_eval.json"))
    ap.add_argument("--icp-iters", type=int, default=30)
    ap.add_argument("--note", default="", help="free text kept in the result (date, visit)")
    ap.add_argument("--only", default="", help="comma-separated run names: run these alone and merge them into the JSON at PATH")
    a = ap.parse_args()
    _lib.require_gpu()
    real, synthetic = clouds()
    every = real + synthetic
    cfg0 = SE.Config()
    res = {"tool": "tools/partial_view_eval.py", "note": a.note, "device": torch.cuda.get_device_name(0),
           "clouds_real": len(real), "clouds_synthetic": len(synthetic), "features": "fpfh", "seed": cfg0.random_seed,
           "view": {"fov_deg": cfg0.view_fov_deg, "size": cfg0.view_size, "distance": cfg0.view_distance,
                    "point_size_voxels": cfg0.view_point_size, "depth_tol_voxels": cfg0.view_depth_tol},
           "runs": {}, "not_measured": ["other seeds", "more than one pose per cloud", "the network's descriptors",
                                        "--verify-score forward (harness.py is out of scope)", "any real scan"]}
    only = [n for n in a.only.split(",") if n]
    if only:
        with open(a.json) as f:
            res = json.load(f)
        res["note_" + "_".join(only)] = a.note
    for view in (False, True):
        for est, opts in RUNS.items():
            if only and est not in only:
                continue
            stat = {}
            key = "%s_%s" % (est, "partial" if view else "full")
            try:
                out = SE.evaluate(None, every, SE.Config(features="fpfh", partial_view=view, **opts), stat=stat)
            except _lib.CorsairHipError as e:      # sc2 refuses a list above 32 768 pairs (whole copies at k = 5)
                res["runs"][key] = {"refused": str(e)}
                print(key, res["runs"][key], file=sys.stderr)
                continue
            res["runs"][key] = report(out, "ransac", len(real))
            if view:
                res["runs"][key]["stat"] = stat["partial_view"]
            print(key, res["runs"][key], file=sys.stderr)
    if not only or PPF_ICP in only:
        behind = "ppf" if "refused" not in res["runs"].get("ppf_partial", {"refused": 1}) else "ppf_v06"
        for view in (False, True):
            out = SE.evaluate(None, every, SE.Config(partial_view=view, icp_max_iter=a.icp_iters, **RUNS[behind]))
            key = "%s_%s" % (PPF_ICP, "partial" if view else "full")
            res["runs"][key] = dict(report(out, "icp", len(real)), icp_iters=a.icp_iters, estimation="point", behind=behind)
            print(key, res["runs"][key], file=sys.stderr)
    if only:
        print(json.dumps(res))
        with open(a.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        return
    # the descriptor estimators only, as in DESIGN 27: ppf has its own ICP row above
    ran = [e for e in RUNS if not e.startswith("ppf") and "refused" not in res["runs"][e + "_partial"]]
    best = max(ran, key=lambda e: (res["runs"][e + "_partial"]["within_15deg"], -res["runs"][e + "_partial"]["rre_deg_median"]))
    out = SE.evaluate(None, every, SE.Config(features="fpfh", partial_view=True, icp_max_iter=a.icp_iters, **RUNS[best]))
    res["icp"] = {"behind": best, "icp_iters": a.icp_iters, "estimation": "point", "before": report(out, "ransac", len(real)),
                  "after": report(out, "icp", len(real))}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
