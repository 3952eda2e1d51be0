"""The Python restatement the GPU tests of the device FASTQ reader use for hc_fastq_counts.n_host_ids (haploconduct_amd/fastq_reader.py:
header_token, plain_id, count_host_ids — the regular expression 0|[1-9][0-9]{0,17} over the header tokens) held against host.Fastq's ids on
the header forms tests/test_gpu_fastq_reader.py lists, so that the GPU test's expectation is checked where there is no GPU.  CPU only."""
import pytest

from haploconduct_amd import fastq_reader as FR
from haploconduct_amd import host

ULONG_MAX = 2 ** 64 - 1
# header line (without its newline) -> (token, plain, the id strtoul(token, NULL, 0) gives)
PLAIN = [(b"@0", b"0", 0), (b"@7", b"7", 7), (b"@123456789012345678", b"123456789012345678", 123456789012345678), (b"@ 12", b"12", 12),
         (b"@12 c", b"12", 12), (b"@12\tc", b"12", 12), (b"@12\r", b"12", 12), (b"@\t \v\f34 x", b"34", 34)]
NOT_PLAIN = [(b"@1234567890123456789", b"1234567890123456789", 1234567890123456789), (b"@007", b"007", 7), (b"@0x1F", b"0x1F", 31),
             (b"@abc", b"abc", 0), (b"@", b"", 0), (b"@-1", b"-1", ULONG_MAX), (b"@+5", b"+5", 5), (b"@12/1", b"12/1", 12),
             (b"@99999999999999999999", b"99999999999999999999", ULONG_MAX), (b"@ ", b"", 0), (b"@010", b"010", 8)]
FORMS = [(h, t, True, i) for h, t, i in PLAIN] + [(h, t, False, i) for h, t, i in NOT_PLAIN]


def _file(headers):
    return b"".join(h + b"\nACGT\n+\nIIII\n" for h in headers)


@pytest.mark.parametrize("header,token,plain,want_id", FORMS, ids=[repr(f[0]) for f in FORMS])
def test_restatement_agrees_with_the_host_reader_on_a_header_form(header, token, plain, want_id, tmp_path):
    assert FR.header_token(header) == token
    assert FR.plain_id(token) is plain
    p = tmp_path / "s.fastq"
    p.write_bytes(_file([header]))
    f = host.Fastq(singles=str(p))
    assert f.read_ids.tolist() == [want_id]
    if plain:  # what the device computes for a plain token: its decimal value
        assert int(token) == want_id
    assert FR.count_host_ids(_file([header])) == (0 if plain else 1)


def test_count_over_a_file_of_all_forms_and_its_cuts(tmp_path):
    text = _file([h for h, _, _, _ in FORMS])
    assert FR.count_host_ids(text) == len(NOT_PLAIN)
    assert FR.count_host_ids(_file([h for h, _, _ in PLAIN])) == 0
    # max_reads cuts in front of the forms that are not plain; an incomplete last record and a last line without a newline
    assert FR.count_host_ids(text, max_reads=len(PLAIN)) == 0
    assert FR.count_host_ids(text, max_reads=len(PLAIN) + 2) == 2
    assert FR.count_host_ids(text + b"@abc\nA\n+") == len(NOT_PLAIN)
    assert FR.count_host_ids(text + b"@abc\nA\n+\nI") == len(NOT_PLAIN) + 1
    assert FR.count_host_ids(b"") == 0
    p = tmp_path / "s.fastq"
    p.write_bytes(text)
    assert host.Fastq(singles=str(p)).read_ids.tolist() == [i for _, _, _, i in FORMS]
