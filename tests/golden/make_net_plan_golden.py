"""Writes tests/golden/net_plan_*.txt: the canonical launch sequence of the planned executor (csrc/net.hip, trace mode) for
the benchmarked networks.  The sequences committed with this script were checked launch for launch - entry point, geometry, data
flow, counter-stream offsets - against the round-2 Python executor they replace (which ran the GPU parity suite green), before
that executor was deleted; regenerate only for a deliberate change of the plan.

    python tests/golden/make_net_plan_golden.py

The variant matrix (VARIANTS below) pins the shipped default configuration and every option that decides which path the planner
takes: three cases as full text (net_plan_variant_*.txt), all the others as a SHA-1 of that text (net_plan_variants.json).

    python tests/golden/make_net_plan_golden.py --variants             # rewrite the variant fixtures
    python tests/golden/make_net_plan_golden.py --add                  # record the digests of the cases net_plan_variants.json lacks
    python tests/golden/make_net_plan_golden.py --print <variant id>   # one case's text on stdout, to diff two builds of the library
    python tests/golden/make_net_plan_golden.py --dump <directory>     # every case's text, one file per variant
    python tests/golden/make_net_plan_golden.py --list                 # the variant ids
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import plan_trace as T  # noqa: E402

CASES = [("G32up-c", 8), ("G32up", 16), ("D32_st3", 8), ("G32up-c@64", 4), ("D32_st3@64", 4)]


def text(which, N):
    # one stream, and the localisation nets as separate modules (the configuration the deleted executor was compared in; the fused
    # localisation launches of csrc/locnet.hip came later and are covered by structure tests + the GPU parity suite)
    # ... and the weight gradients in line on the one stream (option wgrad_stream, round 4, moves them beside the data-gradient chain:
    # same launches, other stream - tests/test_net_plan.py::test_weight_gradients_run_beside_the_data_gradient_chain)
    r = T.trace(which, N, options=[("overlap_groups", 0), ("fuse_locnet", 0), ("pack_overlap", 0), ("head_fuse", 0), ("wgrad_stream", 0)])
    out = [f"# {which} batch {N}: draws {r['draws']}"]
    for phase in ("forward", "backward", "updateGradInput"):
        out.append(f"## {phase}")
        out += T.canon(r[phase])
    return "\n".join(out) + "\n"


# ---- the variant matrix: (network, batch) x (options over the default), plus the data-parallel cases
VARIANT_NETS = [("D32_st3", 8), ("D32_st3", 128), ("D32_st3@64", 4), ("G32up-c", 8), ("G32up-c", 128), ("G32up", 16), ("G32up", 256)]
VARIANT_OPTIONS = [(), (("grouped", 0),), (("stacking", 0),), (("fusion", 0),), (("fuse_locnet", 0),), (("fuse_locnet", 2),), (("view_fuse", 0),),
                   (("cat_fuse", 0),), (("head_fuse", 0),), (("defer_wgrad", 0),), (("share_pool", 0), ("sampler_shared", 0)),
                   (("overlap_groups", 0),), (("wgrad_stream", 0),), (("wino_dsplit", 0),), (("winograd22", 0),), (("winograd22", 1),)]
VARIANT_DP = [(w, 8, dict(world=2, buckets=b)) for w in ("G32up-c", "D32_st3") for b in (True, False)]
FULL_TEXT = ["D32_st3-N8-default", "G32up-c-N8-default", "D32_st3-N8-grouped=0"]      # committed whole; the others as digests
DIGESTS = os.path.join(HERE, "net_plan_variants.json")


def variant_id(which, N, options=(), dp=None, mode=None):
    tag = "+".join(f"{k}={v}" for k, v in options) or "default"
    if dp:
        tag = "world%d-%s" % (dp["world"], "buckets" if dp["buckets"] else "nobuckets") + ("+" + tag if options else "")
    if mode:
        tag = mode + ("+" + tag if options else "")
    return f"{which}-N{N}-{tag}"


# id -> (network, batch, options, dp, keywords of plan_trace.trace that choose another kind of pass)
VARIANTS = {variant_id(w, n, o): (w, n, o, None, {}) for w, n in VARIANT_NETS for o in VARIANT_OPTIONS}
VARIANTS.update({variant_id(w, n, (), dp): (w, n, (), dp, {}) for w, n, dp in VARIANT_DP})

# ---- recorded on the parent commit of the change that split csrc/net.hip in three: the paths no case above reaches
NOFUSION = (("fusion", 0),)
OPTIONS_16 = [(), NOFUSION, (("stacking", 0),), (("wgrad_stream", 0),)]
OPTIONS_D16 = OPTIONS_16 + [(("grouped", 0),), (("fuse_locnet", 0),), (("fuse_locnet", 2),)]
VARIANTS.update({variant_id(w, n, o): (w, n, o, None, {})                      # the 16 px networks
                 for w, opts in (("D32_st3@16", OPTIONS_D16), ("G16up", OPTIONS_16)) for n in (8, 128) for o in opts})
DP2 = dict(world=2, buckets=True)                                              # world 2 off the fused path (G: the unfused sync-BN exchanges)
VARIANTS.update({variant_id(w, 8, NOFUSION, DP2): (w, 8, NOFUSION, DP2, {}) for w in ("G32up-c", "D32_st3")})
# after net:evaluate(): D whole (dropout as a scaling, the head module by module), the generators forward only (their batch-norm backward is refused)
VARIANTS.update({variant_id("D32_st3", 8, o, mode="evaluate"): ("D32_st3", 8, o, None, dict(evaluate=True)) for o in ((), NOFUSION)})
VARIANTS.update({variant_id(w, n, mode="evaluate-forward"): (w, n, (), None, dict(evaluate=True, backward=False)) for w, n in (("G32up-c", 8), ("G32up", 16))})
# forward_pair on 4 and 8 rows + pair_join, the backward continuing the second pass
VARIANTS[variant_id("G32up-c", 8, mode="pair4")] = ("G32up-c", 8, (), None, dict(pair=4))


def variant_text(vid):
    which, N, options, dp, mode = VARIANTS[vid]
    r = T.trace(which, N, options=list(options), dp=dp, **mode)
    out = [f"# {vid}: draws {r['draws']}", "# stats " + " ".join(f"{k}={v}" for k, v in sorted(r["stats"].items()))]
    for phase in ("first_forward", "forward", "backward", "updateGradInput"):
        if phase in r:
            out.append(f"## {phase}")
            out += T.canon(r[phase])
    return "\n".join(out) + "\n"


def variant_file(vid):
    return os.path.join(HERE, "net_plan_variant_%s.txt" % vid.replace("@", "_at_").replace("=", ""))


def digest(txt):
    return hashlib.sha1(txt.encode()).hexdigest()


if __name__ == "__main__":
    if sys.argv[1:2] == ["--list"]:
        print("\n".join(VARIANTS))
    elif sys.argv[1:2] == ["--print"]:
        sys.stdout.write(variant_text(sys.argv[2]))
    elif sys.argv[1:2] == ["--dump"]:          # every case's text into a directory
        os.makedirs(sys.argv[2], exist_ok=True)
        for vid in VARIANTS:
            open(os.path.join(sys.argv[2], vid + ".txt"), "w").write(variant_text(vid))
    elif sys.argv[1:2] == ["--add"]:           # the recorded digests stay as they are
        sums = json.load(open(DIGESTS))
        new = [vid for vid in VARIANTS if vid not in sums and vid not in FULL_TEXT]
        sums.update({vid: digest(variant_text(vid)) for vid in new})
        json.dump(sums, open(DIGESTS, "w"), indent=0, sort_keys=True)
        print(DIGESTS, len(new), "digests added")
    elif sys.argv[1:2] == ["--variants"]:
        sums = {}
        for vid in VARIANTS:
            txt = variant_text(vid)
            if vid in FULL_TEXT:
                open(variant_file(vid), "w").write(txt)
                print(variant_file(vid))
            else:
                sums[vid] = digest(txt)
        json.dump(sums, open(DIGESTS, "w"), indent=0, sort_keys=True)
        print(DIGESTS, len(sums), "digests")
    else:
        for which, N in CASES:
            fn = os.path.join(HERE, "net_plan_%s_N%d.txt" % (which.replace("@", "_at_"), N))
            open(fn, "w").write(text(which, N))
            print(fn)
