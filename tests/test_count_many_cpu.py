"""smash_cli count-many's manifest (one sample per line: ID, r1 files, r2
files, tab separated): blank lines are skipped, a line without its three
columns and an ID listed twice are errors."""
import pytest

import smash_cli


def write(tmp_path, text):
    p = tmp_path / "lane.tsv"
    p.write_text(text)
    return str(p)


def test_manifest_rows_and_blank_lines(tmp_path):
    m = write(tmp_path, "\na\tx_1.fq y_1.fq\tx_2.fq y_2.fq\n\n   \nb\tz_1.fq.gz\tz_2.fq.gz\r\n")
    assert smash_cli.read_manifest(m) == [("a", ["x_1.fq", "y_1.fq"], ["x_2.fq", "y_2.fq"]),
                                          ("b", ["z_1.fq.gz"], ["z_2.fq.gz"])]


@pytest.mark.parametrize("text, what", [
    ("a\tx_1.fq\tx_2.fq\nb\tz_1.fq\n", "lane.tsv:2: expected ID"),          # a missing column
    ("a\tx_1.fq\t\n", "lane.tsv:1: expected ID"),                              # an empty one
    ("a x_1.fq x_2.fq\n", "lane.tsv:1: expected ID"),                          # no tabs
    ("a\tx_1.fq\tx_2.fq\nb\ty_1.fq\ty_2.fq\na\tz_1.fq\tz_2.fq\n", "lane.tsv:3: sample ID 'a'"),
    ("\n\n", "no samples"),
])
def test_manifest_errors(tmp_path, text, what):
    with pytest.raises(SystemExit) as e:
        smash_cli.read_manifest(write(tmp_path, text))
    assert what in str(e.value)
