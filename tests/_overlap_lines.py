"""The overlaps file's lines, restated plainly (no GPU, no native code): where std::getline cuts a text, which lines are PLAIN — the
form the one-pass readers take (Overlap::from_plain_line on the host, parse_plain_line in csrc/hc_text_kernels.hip; the grammar is the
header comment of that file) — and what their thirteen fields read as.  tests/test_overlap_lines_host.py holds this restatement against
the host's two readers; tests/test_gpu_text_reader.py holds the device's reader against it, line by line."""
import random
import re

FIELDS = ("id1", "id2", "pos1", "pos2", "ord", "ori1", "ori2", "perc1", "perc2", "len1", "len2", "type1", "type2")


def split_lines(text):
    """[(begin, length)] of the lines std::getline reads from `text`: they end at '\\n' only, a last piece without one is a line, an
    empty text has none, empty lines count."""
    out, at = [], 0
    while at < len(text):
        nl = text.find(b"\n", at)
        end = len(text) if nl < 0 else nl
        out.append((at, end - at))
        at = end + 1
    return out


_ID = rb"(0|[1-9][0-9]{0,17})"  # decimal, 1 - 18 digits; a leading 0 would be octal to strtoul(.., 0)
_NUM = rb"(-|[0-9]{1,9})"        # "-" reads as 0 (atoi); leading zeros are decimal to atoi
_CH = rb"(.)"                    # one byte, whatever it is: the rules below say which are valid
_PLAIN = re.compile(b"\t".join([_ID, _ID, _NUM, _NUM, _CH, _CH, _CH, _NUM, _NUM, _NUM, _NUM, _CH, _CH]), re.DOTALL)


def plain_fields(line):
    """The thirteen values of a plain line (numbers as ints, one-byte fields as byte values), or None for a line that is not plain."""
    m = _PLAIN.fullmatch(line)
    if not m:
        return None
    f = dict(zip(FIELDS, m.groups()))
    o = {k: (0 if f[k] == b"-" else int(f[k])) for k in ("id1", "id2", "pos1", "pos2", "perc1", "perc2", "len1", "len2")}
    o.update({k: f[k][0] for k in ("ord", "ori1", "ori2", "type1", "type2")})
    if f["pos2"] == b"-":  # src/Overlap.h:55-59, before the range test
        o["perc2"] = o["len2"] = 0
    if o["ori1"] not in b"+-" or o["ori2"] not in b"+-":
        return None
    if o["perc1"] > 100 or o["perc2"] > 100:
        return None
    if o["type1"] not in b"sp" or o["type2"] not in b"sp":
        return None
    if o["ord"] not in (b"-" if b"s"[0] in (o["type1"], o["type2"]) else b"12"):
        return None
    return o


def perc_of(o):
    """Overlap::get_perc of a restated line."""
    return (o["perc1"] + o["perc2"]) // 2 if o["perc2"] > 0 else o["perc1"]


BASE = [b"12", b"345", b"7", b"9", b"1", b"+", b"-", b"97", b"88", b"150", b"140", b"p", b"p"]
_IDS = [b"0", b"1", b"00", b"01", b"9" * 18, b"1234567890123456789", b"18446744073709551615", b"", b"-", b"-1", b"+1", b"0x1f", b" 1", b"1 ",
        b"1\r", b"1\x00", b"\xb1", b"1e3"]
_NUMS = [b"-", b"0", b"00", b"007", b"9" * 9, b"1234567890", b"", b"--", b"-5", b"5-", b"+5", b" 5", b"5 ", b"0x5", b"5.0", b"\xb5"]
_PERCS = [b"100", b"101", b"000100", b"255", b"4294967396"]
_CHARS = [b"+", b"-", b"1", b"2", b"s", b"p", b"S", b"", b"++", b" ", b"\t", b"\x00", b"\xab"]
_EDGES = {"id1": _IDS, "id2": _IDS, "pos1": _NUMS, "pos2": _NUMS, "ord": _CHARS, "ori1": _CHARS, "ori2": _CHARS, "perc1": _NUMS + _PERCS,
          "perc2": _NUMS + _PERCS, "len1": _NUMS, "len2": _NUMS, "type1": _CHARS, "type2": _CHARS}


def corpus():
    """A deterministic list of lines (bytes, none holds a newline): one valid line, each of its fields replaced in turn by every entry of
    that field's edge list, the ORD x TYPE table, and whole-line malformations."""
    def with_(**kw):
        f = list(BASE)
        for k, v in kw.items():
            f[FIELDS.index(k)] = v
        return b"\t".join(f)

    lines = [with_()]
    for k in FIELDS:
        lines += [with_(**{k: v}) for v in _EDGES[k]]
    lines += [with_(ord=o, type1=t1, type2=t2) for o in (b"-", b"1", b"2", b"+") for t1 in (b"s", b"p") for t2 in (b"s", b"p")]
    lines += [with_(pos2=b"-", perc2=b"101"), with_(pos2=b"-", perc2=b"55", len2=b"66")]
    base = with_()
    lines += [b"\t".join(BASE[:12]), base + b"\tp"]                                          # 12 and 14 fields
    lines += [base + b"\t", b"\t" + base, base.replace(b"\t", b" "), base + b"\r", base + b" "]
    lines += [b"", b"\t" * 12, b"x"]
    lines += [with_(id2=BASE[0])]                                                            # a self overlap
    assert not any(b"\n" in ln for ln in lines)
    return lines


def mutated(seed, n):
    """n valid lines (str), most of them then mutated character by character: inserted or overwritten junk."""
    rng = random.Random(seed)

    def valid():
        t1, t2 = rng.choice("sp"), rng.choice("sp")
        ss = t1 == t2 == "s"
        return "\t".join([str(rng.choice([0, 7, 10, 123456, 99999999, 123456789012345678])), str(rng.randrange(5000)),
                          str(rng.randrange(300)), "-" if ss else str(rng.randrange(300)), rng.choice("12") if t1 == t2 == "p" else "-",
                          rng.choice("+-"), rng.choice("+-"), str(rng.randrange(101)), "-" if ss else str(rng.randrange(101)),
                          str(rng.randrange(1, 999999999)), "-" if ss else str(rng.randrange(500)), t1, t2])

    junk = ["\t", " ", "0", "9", "-", "+", "x", "s", "p", "1", "\r", "00", "1234567890", "0x1f", "101", ""]
    out = []
    for _ in range(n):
        line = valid()
        for _ in range(rng.choice([0, 0, 1, 1, 2, 4])):
            k = rng.randrange(len(line) + 1)
            line = line[:k] + rng.choice(junk) + line[k + rng.choice([0, 1, 1]):]
        out.append(line)
    return out
