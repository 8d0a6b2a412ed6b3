"""The host generator (mktfhe_amd/csrc/client.cpp) judged two-sidedly: every key component and fresh ciphertext is opened under the
party's secrets by tests/ref_keys.py (exact integers, no product code) and its noise, masks, ternary / block-binary draws and
secrets are held against the laws the reference states -- too little noise, the wrong sigma on one component, a stream feeding two
places, a truncating cast or a biased draw fail here, where "gates decrypt" and the one-sided 6 sigma bound pass.  Thresholds:
ref_keys.ALPHA (derived there, never tuned on the generator's output).  Sets: the shipped gadgets and noise at reduced n."""
import numpy as np
import pytest

import ref_keys as R
from helpers import mk

_checks = [0]


def check(ps, what):
    for name, pv in ps.items():
        _checks[0] += 1
        assert pv >= R.ALPHA, (what, name, "p = %.3g < %.3g" % (pv, R.ALPHA))


def bounded(e, sigma, what):
    worst = int(np.abs(e).max())
    assert worst <= 6 * sigma + 1, (what, "max|e|", worst, "sigma", sigma)


# one reduced set per scheme and ring width; n chosen so that the bootstrapping rows give >= 5e4 residuals at the shipped N
SETS = [
    mk.CGGIparam.scaled(n=16), mk.CGGIparam.scaled(n=16, k=2), mk.Blockparam.scaled(n=18, blk_d=6),
    mk.Blockparam.scaled(n=150, N=64, k=3, blk_d=50),                                   # n > 2 N: the LWE key spans all three ring keys
    mk.CCS2party.scaled(n=20), mk.CCS16party.scaled(n=16), mk.CCS8party_N2048.scaled(n=16),
    mk.KMS2party.scaled(n=16), mk.KMS32party.scaled(n=8), mk.KMS2partyblock.scaled(n=18, blk_d=6), mk.KMS2party_N1024_l2.scaled(n=32),
    mk.CGGIparam.scaled(n=64, N=16), mk.KMS2party.scaled(n=64, N=16), mk.CGGIparam.scaled(n=3, N=4096), mk.KMS2party.scaled(n=3, N=4096),
]
ENCRYPTIONS = 20_000
POOL = 50_000          # residuals wanted of the small components (public key, rlk): pooled over secrets-only keys, at most 20 of them


def _ring_keys(p, k):
    out, i = [], 0
    while k.ringkey(i) is not None:
        out.append(np.array(k.ringkey(i)))
        i += 1
    return out


def _open_party(p, crs, k, heavy=True):
    """every component of one party's keys -> {component: opened}"""
    z, s = _ring_keys(p, k), np.array(k.lwekey)
    o = {}
    if heavy:
        if p.scheme == mk.CCS:
            o["brk"] = R.open_ccs_brk(p, k.brk, crs, s, z[0])
        else:
            o["brk"] = R.open_rgsw(p, k.brk, s, z)
        o["ksk"] = R.open_ksk(p, k.ksk, s, z)
    if p.multikey:
        uni = z[1] if p.scheme in (mk.KMS, mk.KMS_BLOCK) else z[0]
        o["pub"] = R.open_pubkey(p, k.pubkey, crs, uni)
        if p.scheme in (mk.KMS, mk.KMS_BLOCK):
            o["rlk"] = R.open_unienc(p, k.rlk_d, k.rlk_f, crs, uni, z[0])           # UniEnc of the GSW ring key under the uni key
    return o


def judge_keys(p, crs, full, extra, enc_seed, encryptions=ENCRYPTIONS):
    """full: parties' complete keys of ONE seed; extra: secrets-only keys (other seeds) that only lengthen the public-key / rlk pools"""
    N, W, name = p.N, p.W, f"{p.name}-n{p.n}-N{p.N}"
    opened = [_open_party(p, crs, k) for k in full] + [_open_party(p, crs, k, heavy=False) for k in extra]
    # ---- noise, per component
    comp = {}
    for o in opened:
        if "brk" in o and p.scheme == mk.CCS:
            comp.setdefault("brk d", []).append(o["brk"]["e_d"]); comp.setdefault("brk f", []).append(o["brk"]["e_f"])
        elif "brk" in o:
            comp.setdefault("brk", []).append(o["brk"]["e"])
        if "pub" in o:
            comp.setdefault("public key", []).append(o["pub"]["e"])
        if "rlk" in o:
            comp.setdefault("rlk_d", []).append(o["rlk"]["e_d"]); comp.setdefault("rlk_f", []).append(o["rlk"]["e_f"])
    comp = {c: np.concatenate(v) for c, v in comp.items()}
    for c, e in comp.items():
        bounded(e, p.beta, (name, c))
        check(R.noise_stats(e, p.beta), (name, c))
    ksk_e = np.stack([o["ksk"]["e"][o["ksk"]["live"]] for o in opened if "ksk" in o])          # [party][live (c, j)][d][t]
    bounded(ksk_e, p.alpha, (name, "ksk"))
    check(R.noise_stats(ksk_e.reshape(-1, p.f), p.alpha), (name, "ksk"))
    for t in range(p.f):                                                                     # all f levels, each on its own
        st = R.noise_stats(ksk_e[..., t].ravel(), p.alpha)
        check({k: st[k] for k in ("mean", "variance")}, (name, "ksk level %d" % t))
    # ---- fresh encryptions under party 0
    bits = np.arange(encryptions) & 1
    ct = np.stack([mk.lwe_ith_encrypt(int(b), 0, full[0], p, deterministic_seed=enc_seed + j) for j, b in enumerate(bits)])
    enc_a, enc_e = R.open_lwe(p, ct, 0, np.array(full[0].lwekey), bits)
    bounded(enc_e, p.alpha, (name, "encryption"))
    check(R.noise_stats(enc_e, p.alpha), (name, "encryption"))
    # ---- masks: uniform words
    ring_masks = [o["brk"]["masks"].reshape(-1, N) for o in opened if "brk" in o] + [o["rlk"]["masks"] for o in opened if "rlk" in o]
    if crs is not None:
        check(R.uniform_stats(crs, W), (name, "CRS"))
        ring_masks.append(R.words(crs, W))
    check(R.uniform_stats(np.concatenate(ring_masks), W), (name, "ring masks"))
    lwe_rows = np.concatenate([o["ksk"]["masks"][o["ksk"]["live"]].reshape(-1, p.n) for o in opened if "ksk" in o] + [enc_a])
    check(R.uniform_stats(lwe_rows, 32), (name, "LWE masks"))
    # ---- independence, whatever the stream layout: (a) no mask is produced twice, by any component of any party
    polys = np.concatenate(ring_masks)
    if W == 64:
        assert R.count_equal_words([polys]) == 0, (name, "a 64-bit mask word occurs twice")
    assert R.count_equal_rows(polys) == 0, (name, "a mask polynomial occurs twice")
    if 32 * p.n >= 64:
        assert R.count_equal_rows(lwe_rows) == 0, (name, "an LWE mask row occurs twice")
    # (b) no noise vector is produced twice, and no two are correlated
    noise_rows = np.concatenate(list(comp.values()))
    assert R.count_equal_rows(noise_rows) == 0, (name, "a noise polynomial occurs twice")
    check({"noise rows": R.cross_correlation(noise_rows)}, (name, "cross-correlation"))
    levels = np.concatenate([np.moveaxis(k, -1, 0).reshape(p.f, -1) for k in ksk_e])           # one vector per party and level
    assert R.count_equal_rows(levels) == 0, (name, "two key-switching levels carry the same noise")
    check({"ksk levels": R.cross_correlation(levels)}, (name, "cross-correlation"))
    # (c) one ternary r per key bit / per rlk, all different, uniform on {-1, 0, 1}
    rs = [o["brk"]["r"] for o in opened if "brk" in o and p.scheme == mk.CCS] + [o["rlk"]["r"][None] for o in opened if "rlk" in o]
    if rs:
        rs = np.concatenate(rs)
        assert R.count_equal_rows(rs) == 0, (name, "a ternary r is used twice")
        check({"ternary r": R.ternary_uniform(rs)}, (name, "r"))
    return comp


def _keys_of(p, seed):
    crs = mk.CRS(p, seed) if p.multikey else None
    full = [mk.party_keygen(crs, p, party=i, deterministic_seed=seed) for i in range(min(p.nparty, 2))]
    extra = []
    if p.multikey:
        have = len(full) * p.l_uni * p.N
        while have < POOL and len(extra) < 20:
            extra.append(mk.party_keygen(crs, p, party=len(extra) % p.nparty, secrets_only=True, deterministic_seed=seed + 1 + len(extra)))
            have += p.l_uni * p.N
    return crs, full, extra


@pytest.mark.parametrize("p", SETS, ids=lambda p: f"{p.name}-n{p.n}-N{p.N}-k{p.k}")
def test_host_keys_and_ciphertexts_follow_their_laws(p):
    """every component opens exactly under the secrets with max|e| <= 6 sigma + 1, and every statistic of ref_keys passes per
    component: bootstrapping rows, d, f, public key, rlk_d, rlk_f, key-switching rows (pooled and per level, all f of them), fresh
    encryptions; masks and CRS uniform; no mask, noise vector or ternary r produced twice, no two noise vectors correlated"""
    crs, full, extra = _keys_of(p, seed=4100 + SETS.index(p))
    comp = judge_keys(p, crs, full, extra, enc_seed=900_000)
    if p.N >= 1024 or p.N == 64:
        assert all(e.size >= POOL for e in comp.values()), {c: e.size for c, e in comp.items()}


def test_fresh_entropy_keys_follow_the_same_laws():
    """deterministic_seed=None: the same judgement on keys nobody can reproduce, and two calls share no mask polynomial"""
    p = mk.KMS2party.scaled(n=8, N=256)
    crs = mk.CRS(p)
    sets = []
    for _ in range(2):
        full = [mk.party_keygen(crs, p, party=i) for i in range(2)]
        z = [_ring_keys(p, k) for k in full]
        sets.append(np.concatenate([R.open_rgsw(p, k.brk, np.array(k.lwekey), zz)["masks"].reshape(-1, p.N) for k, zz in zip(full, z)]))
    assert R.count_equal_words(sets) == 0 and R.count_equal_rows(np.concatenate(sets)) == 0
    opened = [_open_party(p, crs, k) for k in full]
    for i, o in enumerate(opened):
        for c, e in (("brk", o["brk"]["e"]), ("public key", o["pub"]["e"]), ("rlk_d", o["rlk"]["e_d"]), ("rlk_f", o["rlk"]["e_f"])):
            bounded(e, p.beta, ("fresh", i, c))
            check(R.noise_stats(e, p.beta), ("fresh", i, c))
        e = o["ksk"]["e"][o["ksk"]["live"]]
        bounded(e, p.alpha, ("fresh", i, "ksk"))
        check(R.noise_stats(e.reshape(-1, p.f), p.alpha), ("fresh", i, "ksk"))
        check(R.uniform_stats(o["brk"]["masks"], p.W), ("fresh", i, "ring masks"))
    ct = np.stack([mk.lwe_ith_encrypt(j & 1, 1, full[1], p) for j in range(4000)])
    a, e = R.open_lwe(p, ct, 1, np.array(full[1].lwekey), np.arange(4000) & 1)
    bounded(e, p.alpha, "fresh encryption")
    check(R.noise_stats(e, p.alpha), "fresh encryption")
    assert R.count_equal_rows(a) == 0
    noise = np.concatenate([np.concatenate([o["brk"]["e"], o["pub"]["e"], o["rlk"]["e_d"], o["rlk"]["e_f"]]) for o in opened])
    assert R.count_equal_rows(noise) == 0
    check({"noise rows": R.cross_correlation(noise)}, "fresh cross-correlation")


def test_encryption_under_party_i_leaves_the_other_blocks_zero():
    """lwe_ith_encrypt (scheme.jl:370-386) on a 4-party set: the mask sits in party i's block, every other block is zero word for
    word, and the ciphertext opens under party i's key alone"""
    p = mk.KMS4party.scaled(n=12, N=64)
    crs = mk.CRS(p, 31)
    keys = [mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=31) for i in range(4)]
    for i in range(4):
        bits = np.arange(64) & 1
        ct = np.stack([mk.lwe_ith_encrypt(int(b), i, keys[i], p, deterministic_seed=7000 + 100 * i + j) for j, b in enumerate(bits)])
        a, e = R.open_lwe(p, ct, i, np.array(keys[i].lwekey), bits)                  # asserts the zero blocks
        assert ct.shape[1] == 4 * p.n + 1 and a.all(axis=None) and R.count_equal_rows(a) == 0
        bounded(e, p.alpha, ("party", i))
        for o in range(4):
            if o != i:
                assert not ct[:, o * p.n:(o + 1) * p.n].any()


def _secret_pool(p, seeds):
    crs = mk.CRS(p, 1) if p.multikey else None
    return [mk.party_keygen(crs, p, party=0, secrets_only=True, deterministic_seed=s) for s in seeds]


def test_secret_keys_follow_their_laws():
    """pooled over secrets-only keys, >= 1e4 draws per law: binary LWE and ring keys have binomial weight; block-binary keys hold at
    most one 1 per block with the index uniform on 0..blk_len for blk_len 2, 3, 4"""
    ks = _secret_pool(mk.CGGIparam, range(200, 216))
    check({"LWE key": R.binary_weight(np.stack([k.lwekey for k in ks])), "ring key": R.binary_weight(np.stack([k.ringkey(0) for k in ks]))}, "CGGI secrets")
    assert R.count_equal_rows(np.stack([k.lwekey for k in ks])) == 0 and R.count_equal_rows(np.stack([k.ringkey(0) for k in ks])) == 0
    q = mk.KMS2party.scaled(n=64, N=256)
    ks = _secret_pool(q, range(300, 340))
    check({"gsw ring key": R.binary_weight(np.stack([k.ringkey(0) for k in ks])), "uni ring key": R.binary_weight(np.stack([k.ringkey(1) for k in ks]))}, "KMS secrets")
    assert R.count_equal_rows(np.stack([np.concatenate([k.ringkey(0), k.ringkey(1)]) for k in ks])) == 0
    assert not any(np.array_equal(k.ringkey(0), k.ringkey(1)) for k in ks), "the two ring keys of a KMS party are one draw"
    for blk_len in (2, 3, 4):
        b = mk.Blockparam.scaled(n=blk_len * 240, blk_len=blk_len, blk_d=240)
        ks = _secret_pool(b, range(400, 450))                                       # 12 000 blocks
        check({"index": R.block_uniform(np.stack([k.lwekey for k in ks]), blk_len)}, ("block key", blk_len))
        free = np.stack([k.ringkey(0)[b.n:] for k in ks])                           # the ring key beyond the embedded LWE key: fair bits
        check({"free ring bits": R.binary_weight(free)}, ("block key", blk_len))


@pytest.mark.parametrize("p", [mk.Blockparam.scaled(n=18, N=64, blk_d=6), mk.Blockparam.scaled(n=150, N=64, k=3, blk_d=50),
                               mk.Blockparam.scaled(n=128, N=64, k=2, blk_len=2, blk_d=64), mk.KMS2partyblock.scaled(n=18, N=64, blk_d=6),
                               mk.CGGIparam.scaled(n=32, N=64, k=2), mk.CCS2party.scaled(n=32, N=64), mk.KMS2party.scaled(n=32, N=64)],
                         ids=lambda p: f"{p.name}-n{p.n}-k{p.k}")
def test_ring_keys_embed_the_lwe_key_exactly_where_the_reference_says(p):
    """LMSS: ring key coefficient c N + i IS lwekey[c N + i] below n (key.jl:52-69), also for n > N and k = 3; KMS_block: the uni key
    embeds the LWE key, the GSW key does not; CGGI / CCS / KMS ring keys are draws of their own; parties of one seed differ"""
    crs = mk.CRS(p, 9) if p.multikey else None
    keys = [[mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=s) for i in range(p.nparty)] for s in range(500, 520)]
    N, n = p.N, p.n
    agree = {}                                    # ring key index -> positions where it equals the LWE key, over all keys
    for ks in keys:
        for k in ks:
            s, z = np.array(k.lwekey), _ring_keys(p, k)
            flat = np.concatenate(z)
            if p.scheme == mk.LMSS:
                assert np.array_equal(flat[:n], s), "LMSS ring key does not embed the LWE key"
            elif p.scheme == mk.KMS_BLOCK:
                assert np.array_equal(z[1][:n], s), "KMS_block uni key does not embed the LWE key"
                agree.setdefault(0, []).append(z[0][:n] == s)
            else:
                for c, zc in enumerate(z):
                    m = min(n, N)
                    agree.setdefault(c, []).append(zc[:m] == s[:m])
        if p.nparty > 1:
            assert not np.array_equal(ks[0].lwekey, ks[1].lwekey) and not np.array_equal(ks[0].ringkey(0), ks[1].ringkey(0)), "parties of one seed share secrets"
    for c, a in agree.items():                    # independent fair bits agree half the time
        a = np.concatenate(a)
        check({"agreement": R.p_of_z((a.sum() - a.size / 2.0) / np.sqrt(a.size / 4.0))}, (p.name, "ring key", c, "vs LWE key"))


def test_zz_the_number_of_checks_is_within_the_budget():
    """ref_keys.ALPHA is BUDGET / CHECKS: the checks this module made must not outnumber the CHECKS it was derived for"""
    assert _checks[0] <= R.CHECKS, _checks[0]
    print("p-value checks:", _checks[0])
