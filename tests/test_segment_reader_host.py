"""The native segment_*.tsv reader of the clustering stage (fhost_read_segment behind cluster_prep.read_segment_arrays) against
the pinned Python mirror, cluster_prep.read_segment() (tests/test_cluster_host.py holds that to the reference's own fixtures): reads,
segs, the gaps / softclip / poly dicts, tail categories, and -- through a host-side grouping of the (I row, token stream) keys
written here -- read_reps.  Every decline reason: the wrapper yields what the mirror yields and raises what it raises.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_util as cu
from freddie_amd import cluster_prep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_groups(arrays):
    """Context.group_reads()'s arrays, made on the host: reads of a tint with equal (I row, token stream) share a rep, reps in
    first-occurrence order, members ascending."""
    a = arrays.a
    T = a["n_tint"]
    rep_off, read_rep, mem_off, mem, first = [0], [], [0], [], []
    for t in range(T):
        r0, r1, M = int(a["read_off"][t]), int(a["read_off"][t + 1]), int(a["n_seg"][t])
        LW = max((M + 15) // 16, 1)
        words = a["labels"][int(a["lab_off"][t]):int(a["lab_off"][t + 1])].reshape(r1 - r0, LW)
        irow = words & 0x55555555 & ~(words >> 1)
        seen, members = {}, []
        for i in range(r1 - r0):
            key = (irow[i].tobytes(), a["tok"][int(a["tok_off"][r0 + i]):int(a["tok_off"][r0 + i + 1])].tobytes())
            if key not in seen:
                seen[key] = len(members)
                members.append([])
            members[seen[key]].append(i)
            read_rep.append(seen[key])
        for m in members:
            first.append(m[0]); mem.extend(m); mem_off.append(len(mem))
        rep_off.append(rep_off[-1] + len(members))
    return dict(n_tint=T, n_reads=len(read_rep), n_reps=len(first), rep_off=np.array(rep_off, np.int64), read_rep=np.array(read_rep, np.int32),
                rep_mem_off=np.array(mem_off, np.int64), rep_mem=np.array(mem, np.int32), rep_first=np.array(first, np.int32))


def mirror_tail(read):
    pt = read["poly_tail"]
    if len(pt) == 1:
        (key, (length, _)), = pt.items()
        if length > 10:
            return 1 if key in ("SA", "ST") else 2
    return 0


def check_against_mirror(paths, threads=3, n_declined=0):
    """read_segment_arrays + host grouping of a batch of files == the mirror, file by file."""
    arrays = cluster_prep.read_segment_arrays(paths, threads)
    assert len(arrays.declined) == n_declined, arrays.declined
    got = cluster_prep.tints_from_arrays(arrays, host_groups(arrays))
    fto = arrays.file_tint_off.tolist()
    assert len(fto) == len(paths) + 1 and fto[-1] == len(got)
    tails = arrays.a["tail"].tolist()
    for f, path in enumerate(paths):
        want = list(cluster_prep.read_segment(path).values())
        assert got[fto[f]:fto[f + 1]] == want, path
        for t, tint in zip(range(fto[f], fto[f + 1]), want):
            r0 = int(arrays.a["read_off"][t])
            assert tails[r0:r0 + len(tint["reads"])] == [mirror_tail(r) for r in tint["reads"]]
            first = [m[0] for m in tint["read_reps"]]
            assert [tails[r0 + i] for i in first] == cluster_prep.tail_categories(tint).tolist()
    return arrays, got


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text.encode() if isinstance(text, str) else text)
    return str(p)


def test_reference_fixture_files_as_one_batch(tmp_path):
    names = cu.cluster_names()
    assert len(names) == 12
    paths = [cu.segment_tsv_file(n, tmp_path) for n in names]
    arrays, got = check_against_mirror(paths, threads=4)
    assert arrays.a["n_tint"] == 12 and sum(len(t["reads"]) for t in got) == int(arrays.a["read_off"][-1]) > 1000
    assert any(len(m) > 1 for t in got for m in t["read_reps"])                          # the grouping has something to do
    assert any(r["poly_tail"] for t in got for r in t["reads"]) and any(r["softclip"] for t in got for r in t["reads"])
    one, _ = check_against_mirror(paths[:1], threads=1)
    assert one.a["n_tint"] == 1


GOOD = ("#chr1\t7\t100,200,300,400\n"
        "0\tr0\tchr1\t+\t7\t101\t0-2:5,SSC:4,\n"
        "1\tr1\tchr1\t-\t7\t121\t0-2:9,ESC:7,\n")

TWO_TINTS = ("#c.1\t5\t0,10,20,30,40\n"
             "#c.1\t9\t5,6\n"
             "0\ta\tc.1\t+\t5\t1201\t0-3:5,SSC:4,\n"
             "1\tb\tc.1\t+\t9\t1\t\n"
             "2\tc\tc.1\t+\t5\t1001\t0-3:9,ESC:7,\n"
             "3\td\tc.1\t-\t9\t2\tEA_25:3,ESC:2,\n"
             "4\te\tc.1\t-\t5\t1001\t0-3:11,\n"
             "5\tf\tc.1\t-\t9\t0\tET_30:0,\n"
             "#c.1\t2\t7\n"                                               # one position: no segments, no reads
             "6\tg\tc.1\t-\t5\t1001\tEA_25:3,ESC:2,\n"
             "7\th\tc.1\t-\t5\t1001\tET_30:0,\n")


def test_two_tints_with_interleaved_reads(tmp_path):
    arrays, got = check_against_mirror([write(tmp_path, "segment_c_5.tsv", TWO_TINTS), write(tmp_path, "segment_e.tsv", "")])
    assert [t["id"] for t in got] == [5, 9, 2] and arrays.file_tint_off.tolist() == [0, 3, 3]
    assert got[0]["read_reps"] == [[0, 1], [2], [3, 4]] and got[1]["read_reps"] == [[0], [1, 2]] and got[2]["reads"] == []
    assert [r["id"] for r in got[1]["reads"]] == [1, 3, 5]


def test_gap_shapes_and_key_rules(tmp_path):
    M = 72
    pos = ",".join(str(10 * i) for i in range(M + 1))
    many = "".join("%d-%d:%d," % (i, i + 1, 5 + i) for i in range(70))
    lines = ["#X\t1\t" + pos + "\n"]
    gaps = ["", many, many[:-2] + "9,", "SA_25:3,ET_30:11,", "ET_30:11,SA_25:3,", "EA_11:12,", "SA_11:12,", "0-1:12,", "SA_10:12,ESC:3,",
            "0-1:10,", "0-1:5,", "0-1:11,", "0-1:11,2-3:12,", "2-3:12,0-1:11,", "2-3:11,0-1:12,", "SSC:1,0-1:11,ESC:1073741823,2-3:12,"]
    for i, g in enumerate(gaps):
        lines.append("%d\tread/%d\tX\t%s\t1\t%s\t%s\n" % (i, i, "+-"[i & 1], ("10" * M)[:M], g))
    arrays, got = check_against_mirror([write(tmp_path, "segment_X_1.tsv", "".join(lines))])
    reps = got[0]["read_reps"]
    rep_of = {r: i for i, m in enumerate(reps) for r in m}
    assert len(got[0]["reads"][1]["gaps"]) == 70
    assert rep_of[1] != rep_of[2]                                         # the last token
    assert rep_of[3] != rep_of[4]                                         # poly order
    assert rep_of[5] != rep_of[6] and rep_of[6] != rep_of[7]              # S vs E; a gap token vs a poly token with the same number
    assert rep_of[9] == rep_of[10] != rep_of[11]                          # 10 vs 5: one rep; 10 vs 11: two
    assert rep_of[12] != rep_of[13] and rep_of[12] == rep_of[14] == rep_of[15]     # gap order; the key holds the lengths in line order, nothing else
    assert arrays.a["tail"].tolist() == [0, 0, 0, 0, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]


# (what is wrong, the file, the mirror's exception or None when the file is legal to it, the line that declines it, the reader's reason)
GRAMMAR = "the line does not match the grammar"
DECLINES = [
    ("label 3", GOOD.replace("\t121\t", "\t131\t"), AttributeError, 3, GRAMMAR),
    ("empty line", GOOD + "\n", AttributeError, 4, GRAMMAR + " (a number is missing)"),
    ("no newline at the end", GOOD[:-1], AttributeError, 3, "a line without a newline"),
    ("a space in the name", GOOD.replace("\tr1\t", "\tr 1\t"), AttributeError, 3, "the read name does not match the grammar"),
    ("unknown gap entry", GOOD.replace("ESC:7,", "XSC:7,"), AttributeError, 3, "the gaps field does not match the grammar"),
    ("gap entry without its comma", GOOD.replace("ESC:7,", "ESC:7"), AttributeError, 3, GRAMMAR),
    ("header without positions", GOOD.replace("\t100,200,300,400", "\t"), AttributeError, 1, GRAMMAR + " (a number is missing)"),
    ("non-ASCII byte", GOOD.replace("\tr1\t", "\tr\u00e9\t"), AttributeError, 3, "the read name does not match the grammar"),
    ("positions that do not rise (:131)", GOOD.replace("100,200,300,400", "100,200,200,400"), AssertionError, 1, "segment positions that do not rise (:131)"),
    ("tint id twice (:135)", GOOD + "#chr1\t7\t1,2\n", AssertionError, 4, "a tint id is repeated (:135)"),
    ("label count (:165)", GOOD.replace("\t121\t", "\t12\t"), AssertionError, 3, "the number of labels is not the number of segments (:165)"),
    ("contig of the read (:167)", GOOD.replace("\tr1\tchr1\t", "\tr1\tchr2\t"), AssertionError, 3, "the read's contig is not its tint's (:167)"),
    ("gap beyond the row (:168)", GOOD.replace("0-2:9,", "0-3:9,"), AssertionError, 3, "a gap outside the read's segments (:168)"),
    ("gap with j1 == j2 (:168)", GOOD.replace("0-2:9,", "2-2:9,"), AssertionError, 3, "a gap outside the read's segments (:168)"),
    ("read before its header", "5\tq\tchr1\t+\t8\t1\t\n" + GOOD, KeyError, 1, "a read whose tint has no header yet"),
    ("leading zero in a gap length", GOOD.replace("0-2:9,", "0-2:011,") + "2\tr2\tchr1\t-\t7\t121\t0-2:11,\n", None, 3, "a number with a leading zero"),
    ("leading zero in a read id", GOOD.replace("1\tr1", "01\tr1"), None, 3, "a number with a leading zero"),
    ("number beyond the token encoding", GOOD.replace("0-2:9,", "0-2:1073741824,"), None, 3, "a number that does not fit"),
    ("number beyond 18 digits", GOOD.replace("0-2:9,", "0-2:12345678901234567890,"), None, 3, "a number that does not fit"),
    ("gap key twice", GOOD.replace("0-2:9,", "0-2:9,0-2:30,") + "2\tr2\tchr1\t-\t7\t121\t0-2:30,\n", None, 3, "a gap key twice in one line"),
    ("poly key twice", GOOD.replace("ESC:7,", "SA_20:1,SA_5:2,") + "2\tr2\tchr1\t-\t7\t121\t0-2:9,SA_5:2,\n", None, 3, "a poly-tail key twice in one line"),
    ("CRLF line ends", GOOD.replace("\n", "\r\n"), None, 1, GRAMMAR),
]


@pytest.mark.parametrize("what,text,raises,line,reason", DECLINES, ids=[d[0] for d in DECLINES])
def test_declined_files_behave_as_the_mirror(tmp_path, what, text, raises, line, reason):
    read_arrays = cluster_prep.read_segment_arrays                      # (outside every raises block: a missing entry point is no pass)
    good = write(tmp_path, "segment_good.tsv", TWO_TINTS)
    bad = write(tmp_path, "segment_bad.tsv", text.encode("utf-8"))
    native = read_arrays([good, bad, good], 2, mirror=False)            # the reader alone: it declines this file, here, for this reason
    assert native.declined == [(bad, line, reason)]
    assert native.file_tint_off.tolist() == [0, 3, 3, 6] and native.a["n_tint"] == 6
    native.close()
    if raises is not None:
        with pytest.raises(raises):
            cluster_prep.read_segment(bad)
        with pytest.raises(raises):
            read_arrays([good, bad, good], 2)
        return
    arrays, got = check_against_mirror([good, bad, good], n_declined=1)
    assert arrays.declined == [(bad, line, reason)]
    assert arrays.file_tint_off.tolist() == [0, 3, 4, 7]
    assert got[0:3] == got[4:7]


def test_unreadable_file_raises_as_the_mirror(tmp_path):
    read_arrays = cluster_prep.read_segment_arrays
    missing = str(tmp_path / "segment_none.tsv")
    assert read_arrays([missing], 1, mirror=False).declined == [(missing, 0, "cannot read the file")]
    with pytest.raises(FileNotFoundError):
        read_arrays([missing], 1)


def test_reader_under_asan_ubsan(tmp_path):
    """The same tests on the AddressSanitizer + UndefinedBehaviorSanitizer build of the host library (built and loaded as
    tests/test_sanitizers.py does), in a child interpreter; any report aborts the child."""
    def runtime(name):
        path = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
        return path if os.path.isabs(path) and os.path.exists(path) else None
    asan, ubsan = runtime("libasan.so"), runtime("libubsan.so")
    if not asan or not ubsan:
        pytest.skip("the sanitizer runtimes are not installed")
    host = str(tmp_path / "libfreddie_host_asan.so")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-shared", "-fPIC", "-o", host,
                           os.path.join(ROOT, "freddie_amd", "csrc", "freddie_host.cpp")])
    env = dict(os.environ, LD_PRELOAD=asan + ":" + ubsan, FHOST_LIB=host,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:allocator_may_return_null=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    probe = "import sys; sys.path.insert(0, %r); from freddie_amd import _host; _host.load(); print(open('/proc/self/maps').read())" % ROOT
    maps = subprocess.run([sys.executable, "-c", probe], env=env, capture_output=True, text=True, timeout=300).stdout
    assert "libfreddie_host_asan.so" in maps and "libasan" in maps and "/freddie_amd/libfreddie_host.so" not in maps
    res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "tests/test_segment_reader_host.py", "-k", "not asan"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = res.stdout[-3000:] + res.stderr[-3000:]
    assert res.returncode == 0, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert " passed" in res.stdout and "skipped" not in res.stdout
